"""CPU tests of lzip-compressed SAM input (`lzip x.sam`, `plzip x.sam`: members back to back) through the host reader of the
`slimm` command (`slimm --dump-records` / `--dump-raw`): every lzip copy reads exactly as the plain SAM file does, from a file
and from redirected standard input; a truncated file, trailing data and every other damage are errors that name them, with
status 1; BAM inside is refused in words.  The inputs: tests/sam_lzip.py (the committed files, members written with Python's
`lzma`) and tests/lzip_directed.py; no `lzip` binary is needed.  No GPU is touched."""
import os
import subprocess

import pytest

from tests import lzip_directed as LD
from tests import sam_lzip as Z
from tests.bam_io import write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
REFUSED = b"lzip-compressed input is not supported unless it decodes"


def run(args, **kw):
    return subprocess.run([CLI] + args, capture_output=True, **kw)


_texts = {}


def text_of(tmp_path, grouped, n):
    if (grouped, n) not in _texts:
        _texts[(grouped, n)] = Z.case_text(tmp_path, grouped, n)
    return _texts[(grouped, n)]


def inputs(tmp_path, grouped):
    """{kind: (text, lzip bytes)}: every input kind of that order."""
    tag = "grouped" if grouped else "any"
    out = {k: (text_of(tmp_path, grouped, n), Z.golden(name.format(tag))) for k, (n, name, tags) in Z.GOLDEN_KINDS.items() if tag in tags}
    short = text_of(tmp_path, grouped, 1_000)
    out.update({k: (short, blob) for k, blob in Z.written_copies(short).items()})
    if grouped:
        small = text_of(tmp_path, True, 50)
        skip = Z.header_len(small)
        # (the directed members in front hold `@CO` lines only: the SAM header's lines come behind them, so the file reads as a
        # header of comments, then the header proper -- which SAM allows in any order)
        out.update({"directed_" + k: (text, blob) for k, (blob, text, _) in LD.INPUTS(small[:skip], small[skip:])[0].items() if k != "header_planted_in_the_payload"})
    return out


@pytest.mark.parametrize("grouped", [True, False])
def test_lzip_sam_reads_as_the_plain_file(tmp_path, grouped):
    """--dump-records and --dump-raw of x.sam.lz equal those of the plain text, for every input kind."""
    for kind, (text, blob) in inputs(tmp_path, grouped).items():
        p = str(tmp_path / "plain.sam")
        open(p, "wb").write(text)
        plain = run(["--dump-records", p])
        assert plain.returncode == 0 and plain.stdout.startswith(b"#format\tSAM"), (kind, plain.stderr[-500:])
        q = str(tmp_path / f"x.{kind}.sam.lz")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert got.returncode == 0, (kind, got.stderr[-500:])
        assert got.stdout == plain.stdout and got.stderr == plain.stderr, kind
        for window_mb in (1, 3):
            r = run(["--dump-raw", "--window-mb", str(window_mb), q])
            assert r.returncode == 0 and r.stdout == text[Z.header_len(text):], (kind, window_mb, r.stderr[-500:])


def test_lzip_sam_from_redirected_standard_input(tmp_path):
    """`slimm --dump-records /dev/stdin < x.sam.lz`.  (Through a real pipe no form is read today: DESIGN section 9.)"""
    text = text_of(tmp_path, True, 3_000)
    p = str(tmp_path / "plain.sam")
    open(p, "wb").write(text)
    plain = run(["--dump-records", p])
    q = os.path.join(Z.GOLDEN, "config1_grouped_m17.sam.lz")
    got = run(["--dump-records", "/dev/stdin"], stdin=open(q, "rb"))
    assert got.returncode == 0 and got.stdout == plain.stdout, got.stderr[-500:]


def test_damage_and_what_is_not_taken_are_errors_that_say_so(tmp_path):
    """A truncated file, trailing data, and every other damage and refused directed input: status 1, the words, the file's name."""
    good, cases = Z.damaged(text_of(tmp_path, True, 1_000))
    small = text_of(tmp_path, True, 50)
    skip = Z.header_len(small)
    cases = {k: (b, w.encode()) for k, (b, w) in cases.items() if k not in ("not_lzip", "inside_the_magic")}   # (those are no lzip files to the command, which tells one by LZIP and a version byte)
    cases.update({"directed_" + k: (b, LD.REFUSED[k].encode()) for k, b in LD.INPUTS(small[:skip], small[skip:])[1].items()})
    assert {"inside_the_stream", "trailing_data"} <= set(cases)
    for name, (data, word) in cases.items():
        q = str(tmp_path / f"{name}.sam.lz")
        open(q, "wb").write(data)
        for args in (["--dump-records", q], ["--dump-raw", q]):
            r = run(args)
            assert r.returncode == 1 and REFUSED in r.stderr and word in r.stderr and r.stderr.rstrip().endswith(q.encode()), (name, args[0], r.stderr[-300:])


def test_an_lzip_stream_that_holds_bam_is_refused(tmp_path):
    from tests.cases import tiny_case
    w = tiny_case()
    p = str(tmp_path / "x.bam")
    write_bam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    import gzip
    inner = gzip.decompress(open(p, "rb").read())   # (the BGZF members inflated: the BAM stream)
    assert inner[:4] == b"BAM\1"
    q = str(tmp_path / "x.bam.lz")
    open(q, "wb").write(Z.member(inner))
    r = run(["--dump-records", q])
    assert r.returncode == 1 and b"an lzip stream that holds BAM: BAM is read from BGZF blocks only" in r.stderr, r.stderr
