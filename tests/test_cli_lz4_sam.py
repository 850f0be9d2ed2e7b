"""CPU tests of lz4-compressed SAM input (`lz4 x.sam`, `lz4 -BD`, frames back to back, skippable frames) through the host reader
of the `slimm` command (`slimm --dump-records` / `--dump-raw`): every lz4 copy reads exactly as the plain SAM file does, from a
file and from standard input; damage is an error that names it; what the reader does not take -- a dictionary, the legacy format, BAM
inside -- is refused in words.  The inputs: tests/sam_lz4.py (the committed compressor-made files, frames written in Python
and the directed inputs; liblz4 is not needed).  No GPU is touched."""
import os
import subprocess

import pytest

from tests import sam_lz4 as L
from tests.bam_io import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
REFUSED = b"lz4-compressed input is not supported unless it decodes"
GOLDEN = {"b4": (3_000, "config1_{}_b4.sam.lz4"), "linked9": (3_000, "config1_{}_linked9.sam.lz4"), "default": (3_000, "config1_{}_default.sam.lz4")}


def run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, **kw)


_texts = {}


def text_of(tmp_path, grouped, n):
    if (grouped, n) not in _texts:
        _texts[(grouped, n)] = L.case_text(tmp_path, grouped, n)
    return _texts[(grouped, n)]


def inputs(tmp_path, grouped):
    """{kind: (text, lz4 bytes)}: every input kind."""
    tag = "grouped" if grouped else "any"
    out = {k: (text_of(tmp_path, grouped, n), L.golden(name.format(tag))) for k, (n, name) in GOLDEN.items()}
    if grouped:
        short = text_of(tmp_path, True, 400)
        out["short"] = (short, L.golden("short_grouped_b4.sam.lz4"))
        out.update({k: (short, blob) for k, blob in L.written_copies(short).items()})
        small = text_of(tmp_path, True, 50)
        skip = L.header_len(small)
        out.update({"directed_" + k: (text, blob) for k, (blob, text, _) in L.INPUTS(small[:skip], small[skip:], staging=False).items()})
    if L.LIB is not None:   # (extra, where the machine has the library)
        text = text_of(tmp_path, grouped, 3_000)
        out["lib_two_frames"] = (text, L.compress(text[:200_000], 5, True, 3) + L.compress(text[200_000:], 4, False, 0, True, True, True))
    return out


@pytest.mark.parametrize("grouped", [True, False])
def test_lz4_sam_reads_as_the_plain_file(tmp_path, grouped):
    """--dump-records and --dump-raw of x.sam.lz4 equal those of the plain text, for every input kind."""
    for kind, (text, blob) in inputs(tmp_path, grouped).items():
        p = str(tmp_path / "plain.sam")
        open(p, "wb").write(text)
        plain = run(["--dump-records", p])
        assert plain.returncode == 0 and plain.stdout.startswith(b"#format\tSAM"), kind
        q = str(tmp_path / f"x.{kind}.sam.lz4")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert got.returncode == 0, (kind, got.stderr[-500:])
        assert got.stdout == plain.stdout and got.stderr == plain.stderr, kind
        for window_mb in (1, 3):
            r = run(["--dump-raw", "--window-mb", str(window_mb), q])
            assert r.returncode == 0 and r.stdout == text[L.header_len(text):], (kind, window_mb, r.stderr[-500:])


def test_lz4_sam_from_standard_input(tmp_path):
    """`slimm --dump-records /dev/stdin < x.sam.lz4`.  (Through a real pipe no form is read today: AlignmentFile::open looks at
    the first bytes and rewinds, which a pipe does not do -- plain SAM and the other codecs lose them too.  DESIGN §9.)"""
    text = text_of(tmp_path, True, 3_000)
    p = str(tmp_path / "plain.sam")
    open(p, "wb").write(text)
    plain = run(["--dump-records", p])
    for kind in ("linked9", "default"):
        q = os.path.join(L.GOLDEN, f"config1_grouped_{kind}.sam.lz4")
        got = run(["--dump-records", "/dev/stdin"], stdin=open(q, "rb"))
        assert got.returncode == 0 and got.stdout == plain.stdout, (kind, got.stderr[-500:])


def flipped(blob, at, bit=0x10):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def test_damage_and_what_is_not_taken_are_errors_that_say_so(tmp_path):
    text = text_of(tmp_path, True, 3_000)
    blob = L.golden("config1_grouped_linked9.sam.lz4")
    fr = L.walk(blob)[0]
    blocks = fr["blocks"]
    plain = L.Frame().stored(text)
    small = text_of(tmp_path, True, 50)
    skip = L.header_len(small)
    cases = {
        "behind_the_magic": (blob[:4], b"frame header at byte 0: truncated"),
        "inside_the_frame_header": (blob[:9], b"frame header at byte 0: truncated"),
        "inside_a_block_header": (blob[:blocks[1]["at"] + 2], b"block header at byte"),
        "inside_a_block": (blob[:blocks[1]["at"] + 500], b"block at byte"),
        "inside_a_block_checksum": (blob[:blocks[1]["sum_at"] + 1], b"truncated"),
        "between_blocks": (blob[:blocks[2]["at"]], b"block header at byte"),
        "inside_the_end_mark": (blob[:fr["end_at"] + 2], b"truncated"),
        "inside_the_content_checksum": (plain.bytes()[:-2], b"checksum at byte"),
        "the_content_checksum_missing": (plain.bytes()[:-4], b"checksum at byte"),
        "header_checksum": (flipped(blob, fr["hc_at"]), b"frame header at byte 0: header checksum mismatch"),
        "block_checksum": (flipped(blob, blocks[3]["sum_at"]), b"block checksum mismatch"),
        "content_checksum": (plain.bytes(wrong_sum=True), b"frame at byte 0: content checksum mismatch"),
        "content_size": (plain.bytes(wrong_size=True), b"frame at byte 0: content size mismatch"),
        "block_over_maximum": (L.frame_header(block_id=4) + (70_000).to_bytes(4, "little") + bytes(70_004), b"a block larger than its maximum"),
        "reserved_flg_bit": (L.frame_header(reserved=1) + bytes(4), b"a reserved bit is set"),
        "reserved_bd_bit": (L.frame_header(bd_reserved=8) + bytes(4), b"a reserved bit is set"),
        "version_0": (L.frame_header(version=0) + bytes(4), b"a frame version other than 1"),
        "dictionary": (L.frame_header(dict_id=5) + bytes(4), b"a dictionary is needed: not supported"),
        "legacy": (L.LEGACY + blob[4:], b"the legacy lz4 format (lz4 -l): not supported"),
        "trailing_garbage": (blob + b"garbage", b"bytes behind the last frame that start no frame"),
    }
    cases.update({"directed_" + k: (b, w.encode()) for k, (b, w) in L.INVALID(small[:skip], small[skip:]).items()})
    for name, (data, word) in cases.items():
        q = str(tmp_path / f"{name}.sam.lz4")
        open(q, "wb").write(data)
        for args in (["--dump-records", q], ["--dump-raw", q]):
            r = run(args)
            assert r.returncode != 0 and REFUSED in r.stderr and word in r.stderr and r.stderr.rstrip().endswith(q.encode()), (name, args[0], r.stderr[-300:])


def test_an_lz4_stream_that_holds_bam_is_refused_and_a_skippable_frame_in_front_stays_zstds(tmp_path):
    from tests.cases import tiny_case
    w = tiny_case()
    p = str(tmp_path / "x.bam")
    write_bam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    import gzip
    inner = gzip.decompress(open(p, "rb").read())   # (the BGZF members inflated: the BAM stream)
    assert inner[:4] == b"BAM\1"
    q = str(tmp_path / "x.bam.lz4")
    open(q, "wb").write(L.Frame().stored(inner).bytes())
    r = run(["--dump-records", q])
    assert r.returncode != 0 and b"an lz4 stream that holds BAM" in r.stderr, r.stderr
    # the two formats share the skippable magic: such a file is the zstd reader's, as before
    q = str(tmp_path / "x.sam.lz4")
    open(q, "wb").write(L.skippable() + L.golden("short_grouped_b4.sam.lz4"))
    r = run(["--dump-records", q])
    assert r.returncode != 0 and b"zstd-compressed input is not supported" in r.stderr, r.stderr
