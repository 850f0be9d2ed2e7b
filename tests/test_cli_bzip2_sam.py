"""CPU tests of bzip2-compressed SAM input (`bzip2 x.sam`, pbzip2 / lbzip2 streams back to back) through the host reader of
the `slimm` command (`slimm --dump-records` / `--dump-raw`): every bzip2 copy reads exactly as the plain SAM file does;
texts built to stress the decoder come out as `bz2.decompress` gives them; damage is an error that names it.  No GPU is
touched."""
import bz2
import os
import random
import subprocess
import zlib

import pytest

from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_bam, write_sam
from tests.cases import q18_apart_case, tiny_case
from tests.sam_bz2 import EOS_MAGIC, flip_bit, get_bits, header_len, magics, set_bits, streams, write_copies
from tests.test_cli_compressed_sam import odd_texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
REFUSED = b"bzip2-compressed input is not supported unless it decodes"

CASES = {
    "tiny": tiny_case,
    "q18_apart": q18_apart_case,
    "config1": lambda: make_workload(CONFIGS["config1"], seed=31),
}


def run(args):
    return subprocess.run([CLI] + args, capture_output=True)


def write_case(tmp_path, name):
    w = CASES[name]()
    p = str(tmp_path / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    return p


@pytest.mark.parametrize("case", sorted(CASES))
def test_bzip2_sam_reads_as_the_plain_file(tmp_path, case):
    p = write_case(tmp_path, case)
    plain = run(["--dump-records", p])
    assert plain.returncode == 0 and plain.stdout.startswith(b"#format\tSAM")
    copies = write_copies(p, str(tmp_path))
    assert sorted(copies) == ["header_blocks", "level1", "level9", "streams"]
    for kind, q in copies.items():
        got = run(["--dump-records", q])
        assert got.returncode == 0, (kind, got.stderr[-500:])
        assert got.stdout == plain.stdout, kind
        assert got.stderr == plain.stderr, kind


@pytest.mark.parametrize("name", ["crlf", "no_final_newline", "crlf_no_final_newline", "blank_lines", "short_line", "empty"])
def test_odd_bzip2_text_reads_as_in_the_plain_file(tmp_path, name):
    text = odd_texts()[name].encode()
    p = str(tmp_path / "x.sam")
    open(p, "wb").write(text)
    plain = run(["--dump-records", p])
    for kind, blob in (("one", bz2.compress(text, 9)), ("streams", streams(text, chunk=97, empty_at=0))):
        q = str(tmp_path / f"x.{kind}.sam.bz2")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert (got.returncode, got.stdout, got.stderr) == (plain.returncode, plain.stdout, plain.stderr), kind


@pytest.mark.parametrize("window_mb", [1, 3])
def test_raw_windows_of_bzip2_sam_are_the_text_behind_the_header(tmp_path, window_mb):
    w = make_workload(CONFIGS["config2"], seed=51, n_records=40_000)
    p = str(tmp_path / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(p, "rb").read()
    want = text[header_len(text):]
    for kind, blob in (("one", bz2.compress(text, 9)), ("streams", streams(text, chunk=300_000, workers=4))):
        q = str(tmp_path / f"x.{kind}.sam.bz2")
        open(q, "wb").write(blob)
        r = run(["--dump-raw", "--window-mb", str(window_mb), q])
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == want, kind
        sizes = [int(ln.split("\t")[1]) for ln in r.stderr.decode().splitlines() if ln.startswith("window")]
        assert sum(sizes) == len(want) and max(sizes) <= window_mb << 20


def stress_texts():
    """Texts that reach the decoder's corners: RLE1 runs at the edges of its count byte, every byte value, and blocks of
    900 k bytes none of which repeats the one before -- a symbol per byte: six Huffman tables and about 18 000
    selectors, near the most a block holds.  Each starts with a line that is no header line, so that --dump-raw hands out all of it."""
    rng = random.Random(5)
    runs = b"x\n" + b"".join(bytes([c]) * n for c, n in zip(b"abcabcabcab", (4, 5, 255, 256, 1000, 259, 260, 3, 4, 1, 4000)))
    every = b"x\n" + bytes(range(256)) * 40 + bytes(range(255, -1, -1)) * 40
    alphabet, noisy = b"ACGTNacgtn0123456789\t", bytearray(b"x\n")
    for _ in range(1_200_000):
        c = rng.choice(alphabet)
        noisy.append(c if c != noisy[-1] else alphabet[(alphabet.index(c) + 1) % len(alphabet)])
    noisy = bytes(noisy)
    return {"runs": runs, "every_byte": every, "six_tables": noisy}


@pytest.mark.parametrize("name", sorted(stress_texts()))
@pytest.mark.parametrize("level", [1, 9])
def test_stress_texts_decode_as_bz2_decompress_gives_them(tmp_path, name, level):
    text = stress_texts()[name]
    blob = bz2.compress(text, level)
    assert bz2.decompress(blob) == text
    q = str(tmp_path / "s.sam.bz2")
    open(q, "wb").write(blob)
    r = run(["--dump-raw", q])
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout == text


def test_six_tables_and_many_selectors_are_in_the_stress_text():
    """(the stress text reaches what it is meant to: six tables and about 18 000 selectors -- bzip2 writes at most 18 002 --
    in its first block)"""
    blob = bz2.compress(stress_texts()["six_tables"], 9)
    b = magics(blob)[0]
    p = b + 48 + 32 + 1 + 24
    used16 = get_bits(blob, p, 16)
    p += 16 + 16 * bin(used16).count("1")
    assert get_bits(blob, p, 3) == 6
    assert get_bits(blob, p + 3, 15) > 17_900


def damaged(text: bytes):
    """{name: (bytes, what stderr must say)}"""
    blob = bz2.compress(text, 9)
    first = magics(blob)[0]
    eos = magics(blob, EOS_MAGIC)[-1]
    out = {
        "truncated": (blob[:len(blob) * 2 // 3], b"truncated"),
        "truncated_eos": (blob[:-3], b"truncated"),
        "huffman_bit": (flip_bit(blob, first + 48 + 32 + 1 + 24 + 16 + 2000), REFUSED + b": block at byte"),
        "block_crc": (flip_bit(blob, first + 48 + 7), b"block CRC mismatch"),
        "combined_crc": (flip_bit(blob, eos + 48 + 3), b"combined CRC mismatch"),
        "orig_ptr": (set_bits(blob, first + 48 + 32 + 1, 24, 0xffffff), b"origPtr out of range"),
        "randomised": (set_bits(blob, first + 48 + 32, 1, 1), b"randomised block"),
        "trailing_bytes": (blob + b"\x00\x01garbage", b"bytes after the last end-of-stream marker"),
    }
    return out


@pytest.mark.parametrize("mode", [["--dump-records"], ["--dump-raw"]])
def test_broken_bzip2_sam_is_an_error_that_names_the_damage(tmp_path, mode):
    p = write_case(tmp_path, "config1")
    text = open(p, "rb").read()
    for name, (data, word) in damaged(text).items():
        q = str(tmp_path / f"{name}.sam.bz2")
        open(q, "wb").write(data)
        r = run(mode + [q])
        assert r.returncode != 0, name
        assert REFUSED in r.stderr and word in r.stderr, (name, r.stderr[-300:])


def test_bzip2_wrapped_bam_is_refused(tmp_path):
    w = tiny_case()
    b = str(tmp_path / "x.bam")
    write_bam(b, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    payload, rest = b"", open(b, "rb").read()
    while rest:
        d = zlib.decompressobj(31)
        payload += d.decompress(rest)
        rest = d.unused_data
    q = str(tmp_path / "x.bam.bz2")
    open(q, "wb").write(bz2.compress(payload))
    r = run(["--dump-records", q])
    assert r.returncode != 0 and b"a bzip2 stream that holds BAM: BAM is read from BGZF blocks only" in r.stderr, r.stderr


def test_a_block_without_byte_values_names_the_cause_and_the_byte(tmp_path):
    """The first block of `BZh91AY&SY` + zero bytes has no byte value in use: refused, at byte 4"""
    q = str(tmp_path / "x.sam.bz2")
    open(q, "wb").write(b"BZh91AY&SY" + b"\x00" * 64)
    r = run(["--dump-records", q])
    assert r.returncode != 0
    assert REFUSED + b": block at byte 4: no byte value in use: " + q.encode() in r.stderr, r.stderr
