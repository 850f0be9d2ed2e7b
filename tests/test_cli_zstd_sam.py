"""CPU tests of zstd-compressed SAM input (`zstd x.sam`, frames back to back, skippable frames) through the host reader of the
`slimm` command (`slimm --dump-records` / `--dump-raw`): every zstd copy reads exactly as the plain SAM file does; damage
is an error that names it; what the reader does not take -- a dictionary, a window of more than 128 MiB, BAM inside -- is
refused in words.  The inputs: tests/sam_zst.py (the committed compressor-made files and frames written in Python; libzstd
is not needed).  No GPU is touched."""
import os
import subprocess

import pytest

from tests import sam_zst as Z
from tests.bam_io import write_bam
from tests.test_cli_compressed_sam import odd_texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
REFUSED = b"zstd-compressed input is not supported unless it decodes"
GOLDEN = {"l3": (3_000, "config1_{}_l3.sam.zst"), "l19": (3_000, "config1_{}_l19.sam.zst"), "wlog10": (400, "short_{}_wlog10.sam.zst")}
WRITTEN = ["raw_blocks", "rle_blocks", "plain_header", "single_segment", "frames", "skippable_first"]


def run(args):
    return subprocess.run([CLI] + args, capture_output=True)


_texts = {}


def text_of(tmp_path, grouped, n):
    if (grouped, n) not in _texts:
        _texts[(grouped, n)] = Z.case_text(tmp_path, grouped, n)
    return _texts[(grouped, n)]


def inputs(tmp_path, grouped):
    """{kind: (text, zstd bytes)}: every input kind."""
    tag = "grouped" if grouped else "any"
    out = {k: (text_of(tmp_path, grouped, n), Z.golden(name.format(tag))) for k, (n, name) in GOLDEN.items()}
    text = text_of(tmp_path, grouped, 3_000)
    out.update({k: (text, blob) for k, blob in Z.written_copies(text).items()})
    if Z.LIB is not None:   # (extra, where the machine has the library)
        out["lib_l1_two_frames"] = (text, Z.compress(text[:200_000], 1) + Z.compress(text[200_000:], 1, 0, False, False))
    return out


@pytest.mark.parametrize("grouped", [True, False])
def test_zstd_sam_reads_as_the_plain_file(tmp_path, grouped):
    """--dump-records and --dump-raw of x.sam.zst equal those of the plain file, for every input kind."""
    plain = {}
    for kind, (text, blob) in inputs(tmp_path, grouped).items():
        if len(text) not in plain:
            p = str(tmp_path / f"x{len(text)}.sam")
            open(p, "wb").write(text)
            plain[len(text)] = run(["--dump-records", p])
            assert plain[len(text)].returncode == 0 and plain[len(text)].stdout.startswith(b"#format\tSAM")
        q = str(tmp_path / f"x.{kind}.sam.zst")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert got.returncode == 0, (kind, got.stderr[-500:])
        assert got.stdout == plain[len(text)].stdout and got.stderr == plain[len(text)].stderr, kind
        for window_mb in (1, 3):
            r = run(["--dump-raw", "--window-mb", str(window_mb), q])
            assert r.returncode == 0 and r.stdout == text[Z.header_len(text):], (kind, window_mb, r.stderr[-500:])


@pytest.mark.parametrize("name", sorted(odd_texts()))
def test_odd_zstd_text_reads_as_in_the_plain_file(tmp_path, name):
    text = odd_texts()[name].encode()
    p = str(tmp_path / "x.sam")
    open(p, "wb").write(text)
    plain = run(["--dump-records", p])
    a, b = text[:len(text) // 2], text[len(text) // 2:]
    for kind, blob in (("one", Z.raw_frame(text, step=97, window_log=10)), ("rle", Z.raw_frame(text, step=1_000, rle=True)),
                       ("frames", Z.raw_frame(a, step=61, window_log=None) + Z.skippable() + Z.raw_frame(b, content_size=False, checksum=False))):
        q = str(tmp_path / f"x.{kind}.sam.zst")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert (got.returncode, got.stdout, got.stderr) == (plain.returncode, plain.stdout, plain.stderr), kind


def flipped(blob, at, bit=0x10):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def test_damage_and_what_is_not_taken_are_errors_that_say_so(tmp_path):
    text = text_of(tmp_path, True, 3_000)
    blob = Z.golden("config1_grouped_l3.sam.zst")
    fr = Z.walk(blob)[0]
    first = next(b for b in fr["blocks"] if b["type"] == 2 and b.get("huf_at") and b.get("fse_at"))
    second = fr["blocks"][1]
    raw = Z.raw_frame(text)
    run_blob, _ = Z.run_frame(text[:5_000], 70_000, b"\n")
    far = run_blob.replace(Z.one_match_block(70_000, 1), Z.one_match_block(70_000, len(text)))
    end = first["at"] + 3 + first["size"] - 1
    cases = {
        "behind_the_magic": (blob[:4], b"frame header at byte 0: truncated"),
        "inside_the_frame_header": (blob[:5], b"frame header at byte 0: truncated"),
        "inside_a_block_header": (blob[:second["at"] + 2], b"block header at byte"),
        "inside_a_huffman_description": (blob[:first["huf_at"] + 3], b"truncated"),
        "inside_an_fse_description": (blob[:first["fse_at"] + 1], b"truncated"),
        "inside_the_sequences": (blob[:first["bits_at"] + 9], b"truncated"),
        "between_blocks": (blob[:second["at"]], b"truncated"),
        "inside_the_checksum": (blob[:-2], b"checksum at byte"),
        "the_checksum_missing": (blob[:-4], b"checksum at byte"),
        "huffman_description": (flipped(blob, first["huf_at"], 0x80), b"block at byte"),
        "fse_description": (flipped(blob, first["fse_at"], 0x0f), b"block at byte"),
        "sequence_stream": (flipped(blob, first["bits_at"] + 20), b"at byte"),
        "padding_bit": (flipped(blob, end, blob[end]), b"does not end on its padding bit"),
        "checksum": (flipped(blob, fr["checksum_at"]), b"content checksum mismatch"),
        "content_size": (Z.raw_frame(text, wrong_size=True), b"content size mismatch"),
        "dictionary": (Z.frame_header(None, False, 17, dict_id=5) + Z.block(0, text[:100], last=True), b"a dictionary"),
        "window_256m": (Z.frame_header(None, False, 28) + Z.block(0, text[:100], last=True), b"a window of more than 128 MiB"),
        "reserved_bit": (flipped(raw, 4, 0x08), b"a reserved bit is set"),
        "reserved_block_type": (flipped(raw, Z.walk(raw)[0]["blocks"][0]["at"], 0x06), b"reserved block type"),
        "block_too_large": (Z.frame_header(None, False, 10) + Z.block(0, text[:2_000], last=True), b"a block larger than its maximum"),
        "offset_in_front_of_the_frame": (far, b"an offset beyond the frame's start or window"),
        "trailing_garbage": (blob + b"garbage", b"bytes behind the last frame that start no frame"),
    }
    for name, (data, word) in cases.items():
        q = str(tmp_path / f"{name}.sam.zst")
        open(q, "wb").write(data)
        for args in (["--dump-records", q], ["--dump-raw", q]):
            r = run(args)
            assert r.returncode != 0 and REFUSED in r.stderr and word in r.stderr, (name, args[0], r.stderr[-300:])


def test_a_zstd_stream_that_holds_bam_and_xz_are_refused(tmp_path):
    from tests.cases import tiny_case
    w = tiny_case()
    p = str(tmp_path / "x.bam")
    write_bam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    import gzip
    inner = b"".join(gzip.decompress(m) for m in [open(p, "rb").read()])   # (the BGZF members inflated: the BAM stream)
    assert inner[:4] == b"BAM\1"
    q = str(tmp_path / "x.bam.zst")
    open(q, "wb").write(Z.raw_frame(inner))
    r = run(["--dump-records", q])
    assert r.returncode != 0 and b"a zstd stream that holds BAM" in r.stderr, r.stderr
    q = str(tmp_path / "x.sam.xz")
    open(q, "wb").write(b"\xfd7zXZ\x00" + bytes(64))
    r = run(["--dump-records", q])
    assert r.returncode != 0 and b"xz-compressed input is not supported" in r.stderr, r.stderr
