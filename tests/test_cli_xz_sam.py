"""CPU tests of xz-compressed SAM input (`xz x.sam`, many blocks, streams back to back with stream padding) through the host
reader of the `slimm` command (`slimm --dump-records` / `--dump-raw`): every xz copy reads exactly as the plain SAM
file does; damage is an error that names it; what the reader does not take -- a filter other than LZMA2, BAM inside -- is
refused in words; the three shapes that earlier tests give the reader (the magic in front of garbage) end as one line with
the words and status 1.  The inputs: tests/sam_xz.py (the committed compressor-made files and containers written in Python;
neither an `xz` binary nor liblzma is needed).  No GPU is touched."""
import os
import subprocess

import pytest

from tests import sam_xz as X
from tests.bam_io import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
REFUSED = b"xz-compressed input is not supported unless it decodes"


def run(args):
    return subprocess.run([CLI] + args, capture_output=True)


_texts = {}


def text_of(tmp_path, grouped, n):
    if (grouped, n) not in _texts:
        _texts[(grouped, n)] = X.case_text(tmp_path, grouped, n)
    return _texts[(grouped, n)]


def inputs(tmp_path, grouped):
    """{kind: (text, xz bytes)}: every input kind."""
    tag = "grouped" if grouped else "any"
    out = {k: (text_of(tmp_path, grouped, n), X.golden(name.format(tag))) for k, (n, name) in X.GOLDEN_KINDS.items()}
    short = text_of(tmp_path, grouped, 1_000)
    out.update({k: (short, blob) for k, blob in X.written_copies(short, tag).items()})
    return out


@pytest.mark.parametrize("grouped", [True, False])
def test_xz_sam_reads_as_the_plain_file(tmp_path, grouped):
    """--dump-records and --dump-raw of x.sam.xz equal those of the plain file, for every input kind."""
    plain = {}
    for kind, (text, blob) in inputs(tmp_path, grouped).items():
        if len(text) not in plain:
            p = str(tmp_path / f"x{len(text)}.sam")
            open(p, "wb").write(text)
            plain[len(text)] = run(["--dump-records", p])
            assert plain[len(text)].returncode == 0 and plain[len(text)].stdout.startswith(b"#format\tSAM")
        q = str(tmp_path / f"x.{kind}.sam.xz")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert got.returncode == 0, (kind, got.stderr[-500:])
        assert got.stdout == plain[len(text)].stdout and got.stderr == plain[len(text)].stderr, kind
        for window_mb in (1, 3):
            r = run(["--dump-raw", "--window-mb", str(window_mb), q])
            assert r.returncode == 0 and r.stdout == text[X.header_len(text):], (kind, window_mb, r.stderr[-500:])


def flipped(blob, at, bit=0x10):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def test_damage_and_what_is_not_taken_are_errors_that_say_so(tmp_path):
    text = text_of(tmp_path, True, 1_000)
    blob = X.written_copies(text, "grouped")["reblocked"]
    s = X.walk(blob)[0]
    b0, b1 = s["blocks"][0], s["blocks"][1]
    ch = b0["chunks"][0]
    cases = {
        "inside_the_stream_header": (blob[:7], b"stream header at byte 0: truncated"),
        "inside_a_block_header": (blob[:b0["at"] + 3], b"block header at byte 12: truncated"),
        "inside_a_chunk": (blob[:ch["at"] + 100], b"truncated"),
        "inside_the_check": (blob[:b0["check_at"] + 2], b"truncated"),
        "between_blocks": (blob[:b1["at"]], b"truncated"),
        "inside_the_index": (blob[:s["index_at"] + 3], b"index at byte"),
        "inside_the_footer": (blob[:-3], b"stream footer at byte"),
        "block_header": (flipped(blob, b0["at"] + 2), b"block header CRC32 mismatch"),
        "check": (flipped(blob, b0["check_at"]), b"check mismatch"),
        "lzma_data": (flipped(blob, ch["at"] + ch["header"] + 40), b"at byte"),
        "index": (flipped(blob, s["index_at"] + 2), b"index CRC32 mismatch"),
        "footer": (flipped(blob, s["footer_at"] + 5), b"footer CRC32 mismatch"),
        "bcj": (X.golden(X.REFUSED_KIND[1].format("grouped")), b"a filter chain other than LZMA2 alone (filter id 4)"),
        "trailing_garbage": (blob + b"garbage!", b"bytes behind the last stream that are neither padding nor a stream"),
    }
    for name, (data, word) in cases.items():
        q = str(tmp_path / f"{name}.sam.xz")
        open(q, "wb").write(data)
        for args in (["--dump-records", q], ["--dump-raw", q]):
            r = run(args)
            assert r.returncode != 0 and REFUSED in r.stderr and word in r.stderr, (name, args[0], r.stderr[-300:])


def test_an_xz_stream_that_holds_bam_is_refused(tmp_path):
    from tests.cases import tiny_case
    w = tiny_case()
    p = str(tmp_path / "x.bam")
    write_bam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    import gzip
    inner = gzip.decompress(open(p, "rb").read())   # (the BGZF members inflated: the BAM stream)
    assert inner[:4] == b"BAM\1"
    q = str(tmp_path / "x.bam.xz")
    open(q, "wb").write(X.stored_chunks(inner, step=60_000))
    r = run(["--dump-records", q])
    assert r.returncode != 0 and b"an xz stream that holds BAM" in r.stderr, r.stderr


@pytest.mark.parametrize("tail", [bytes(64), bytes(range(256)) * 8, b"garbage " * 8])
def test_the_magic_in_front_of_garbage_is_one_line_with_the_words_and_status_1(tmp_path, tail):
    """What earlier tests write for "an xz file": the stream flags' CRC32 does not hold (flags 00 01 in the second shape)."""
    q = str(tmp_path / "x.sam.xz")
    open(q, "wb").write(b"\xfd7zXZ\x00" + tail)
    for args in (["--dump-records", q], ["--dump-raw", q]):
        r = run(args)
        lines = [ln for ln in r.stderr.split(b"\n") if ln]
        assert r.returncode == 1 and len(lines) == 1 and r.stdout == b"", (args, r.stderr)
        assert lines[0].startswith(REFUSED + b": stream header at byte 0: header CRC32 mismatch: "), lines
