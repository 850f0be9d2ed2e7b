"""CPU tests of two corners of bzip2 blocks through the host reader of the `slimm` command: a block whose text repeats itself
(its inverse BWT has several cycles, and the walk from origPtr goes round one of them again and again, as bzip2's own
decoder does) reads as the plain SAM file does; a block longer than its stream's level allows is an error that says so.
No GPU is touched."""
import bz2
import os
import random
import subprocess

from tests.bam_io import write_sam
from tests.cases import tiny_case
from tests.sam_bz2 import header_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
REFUSED = b"bzip2-compressed input is not supported unless it decodes"


def run(args):
    return subprocess.run([CLI] + args, capture_output=True)


def periodic_copy(text: bytes, times: int = 2):
    """(the SAM text with its alignment lines `times` times, a bzip2 copy of it whose blocks repeat themselves: a stream of
    header comments that repeat, the header, then the lines `times` times in one block)"""
    h = header_len(text)
    comments = b"@CO\tsame\n" * 4
    plain = comments + text[:h] + text[h:] * times
    blob = bz2.compress(comments, 9) + bz2.compress(text[:h], 9) + bz2.compress(text[h:] * times, 9)
    assert bz2.decompress(blob) == plain
    return plain, blob


def test_blocks_whose_text_repeats_itself_read_as_the_plain_file(tmp_path):
    w = tiny_case()
    p = str(tmp_path / "t.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    for times in (2, 3):
        plain, blob = periodic_copy(open(p, "rb").read(), times)
        q, z = str(tmp_path / f"x{times}.sam"), str(tmp_path / f"x{times}.sam.bz2")
        open(q, "wb").write(plain)
        open(z, "wb").write(blob)
        want, got = run(["--dump-records", q]), run(["--dump-records", z])
        assert want.returncode == 0 and (got.returncode, got.stdout, got.stderr) == (0, want.stdout, want.stderr)
        raw = run(["--dump-raw", z])
        assert raw.returncode == 0 and raw.stdout == plain[header_len(plain):]


def noisy_text(n: int = 300_000, seed: int = 3) -> bytes:
    """A text with no two equal bytes in a row (RLE1 leaves it as it is), its first line no header line"""
    rng, alphabet, out = random.Random(seed), b"ACGTNacgtn0123456789\t", bytearray(b"x\n")
    for _ in range(n):
        c = rng.choice(alphabet)
        out.append(c if c != out[-1] else alphabet[(alphabet.index(c) + 1) % len(alphabet)])
    return bytes(out)


def too_long_for_level_1(text: bytes) -> bytes:
    """A level-9 stream whose first block holds more than 100 000 bytes, relabelled level 1"""
    blob = bz2.compress(text, 9)
    assert len(text) > 150_000 and blob[:4] == b"BZh9"
    return b"BZh1" + blob[4:]


def test_a_block_longer_than_its_level_allows_is_an_error(tmp_path):
    q = str(tmp_path / "x.sam.bz2")
    open(q, "wb").write(too_long_for_level_1(noisy_text()))
    for mode in (["--dump-records"], ["--dump-raw"]):
        r = run(mode + [q])
        assert r.returncode != 0
        assert REFUSED + b": block at byte 4: block longer than its stream's level allows" in r.stderr, r.stderr[-300:]
