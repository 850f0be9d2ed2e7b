"""CPU tests of compressed SAM input (`bgzip x.sam`, `gzip x.sam`) through the host reader of the `slimm` command
(`slimm --dump-records` / `--dump-raw`): every compressed copy reads exactly as the plain SAM file does -- the same header,
the same records, the same errors -- and what fails to inflate is an error that says so.  No GPU is touched."""
import gzip
import os
import subprocess
import zlib

import pytest

from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_bam, write_sam
from tests.cases import q18_apart_case, tiny_case
from tests.sam_gz import GZIP_TOOL, bgzf, compressed_copies, gzip_members, header_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")

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
def test_compressed_sam_reads_as_the_plain_file(tmp_path, case):
    p = write_case(tmp_path, case)
    plain = run(["--dump-records", p])
    assert plain.returncode == 0 and plain.stdout.startswith(b"#format\tSAM")
    copies = compressed_copies(p, str(tmp_path), seed=7)
    assert len(copies) == (4 if GZIP_TOOL else 3)
    for kind, q in copies.items():
        got = run(["--dump-records", q])
        assert got.returncode == 0, (kind, got.stderr[-500:])
        assert got.stdout == plain.stdout, kind   # header line (SAM, order), references, every record row
        assert got.stderr == plain.stderr, kind   # (the Q18 line)


def test_bgzf_header_spans_blocks_and_lines_straddle_blocks(tmp_path):
    p = write_case(tmp_path, "config1")
    text = open(p, "rb").read()
    plain = run(["--dump-records", p]).stdout
    for seed, (lo, hi) in enumerate(((1, 64), (1000, 5000), (60_000, 65_536))):
        blob = bgzf(text, seed=seed, header_blocks=4, lo=lo, hi=hi)
        q = str(tmp_path / f"x{seed}.sam.gz")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert got.returncode == 0 and got.stdout == plain, got.stderr[-500:]


@pytest.mark.parametrize("window_mb", [1, 3, 64])
@pytest.mark.parametrize("mmap", [True, False])
def test_raw_windows_of_bgzf_sam_are_the_text_behind_the_header(tmp_path, window_mb, mmap):
    """AlignmentFile::read_raw on BGZF SAM (what the command hands to slimm_push_sam_bytes): the windows, concatenated, are
    the text behind the header, whatever the window size, mapped or read."""
    w = make_workload(CONFIGS["config2"], seed=51, n_records=40_000)
    p = str(tmp_path / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(p, "rb").read()
    want = text[header_len(text):]
    q = str(tmp_path / "x.sam.gz")
    open(q, "wb").write(bgzf(text, seed=3))
    flags = ["--window-mb", str(window_mb)] + ([] if mmap else ["--no-mmap"])
    r = run(["--dump-raw"] + flags + [q])
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout == want
    sizes = [int(ln.split("\t")[1]) for ln in r.stderr.decode().splitlines() if ln.startswith("window")]
    assert sum(sizes) == len(want) and max(sizes) <= window_mb << 20
    # ... and plain gzip through read_text
    g = str(tmp_path / "y.sam.gz")
    open(g, "wb").write(gzip_members(text, 3))
    r = run(["--dump-raw"] + flags + [g])
    assert r.returncode == 0 and r.stdout == want, r.stderr[-500:]


def flip_crc(blob: bytes, block: int) -> bytes:
    """The CRC32 of the block-th gzip member / BGZF block altered."""
    b, p = bytearray(blob), 0
    for _ in range(block):
        p += (b[p + 16] | (b[p + 17] << 8)) + 1
    end = p + (b[p + 16] | (b[p + 17] << 8)) + 1
    b[end - 8] ^= 0x5a
    return bytes(b)


@pytest.mark.parametrize("mode", [["--dump-records"], ["--dump-raw"]])
def test_broken_compressed_sam_is_an_error(tmp_path, mode):
    p = write_case(tmp_path, "config1")
    text = open(p, "rb").read()
    blob = bgzf(text, seed=5)
    cases = {
        "bgzf_cut": (blob[:len(blob) * 2 // 3], b"truncated"),
        "bgzf_cut_header": (blob[:20], b"truncated"),
        "bgzf_crc": (flip_crc(blob, 4), b"corrupt"),
    }
    gz = gzip_members(text)
    cases["gzip_cut"] = (gz[:len(gz) * 2 // 3], b"truncated")
    cases["gzip_cut_trailer"] = (gz[:-3], b"truncated")
    bad = bytearray(gz)
    bad[-8] ^= 0x5a
    cases["gzip_crc"] = (bytes(bad), b"corrupt")
    bad = bytearray(gz)
    bad[-1] ^= 0x01   # ISIZE
    cases["gzip_isize"] = (bytes(bad), b"corrupt")
    for name, (data, word) in cases.items():
        q = str(tmp_path / f"{name}.sam.gz")
        open(q, "wb").write(data)
        r = run(mode + [q])
        assert r.returncode != 0 and word in r.stderr, (name, r.returncode, r.stderr[-300:])


def test_gzip_wrapped_bam_and_other_compressions_are_clear_errors(tmp_path):
    w = tiny_case()
    b = str(tmp_path / "x.bam")
    write_bam(b, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    # a BAM's payload re-compressed as one plain gzip member: not BGZF
    payload = b""
    rest = open(b, "rb").read()
    while rest:
        d = zlib.decompressobj(31)
        payload += d.decompress(rest)
        rest = d.unused_data
    q = str(tmp_path / "x.bam.gz")
    open(q, "wb").write(gzip.compress(payload))
    r = run(["--dump-records", q])
    assert r.returncode != 0 and b"plain gzip stream that holds BAM" in r.stderr, r.stderr
    for name, magic in (("bzip2", b"BZh91AY&SY"), ("xz", b"\xfd7zXZ\x00\x00\x04"), ("zstd", b"\x28\xb5\x2f\xfd\x00\x00")):
        q = str(tmp_path / f"x.sam.{name}")
        open(q, "wb").write(magic + b"\x00" * 64)
        r = run(["--dump-records", q])
        assert r.returncode != 0 and f"{name}-compressed input is not supported".encode() in r.stderr, (name, r.stderr)


def odd_texts():
    """SAM texts the reader treats in a particular way: CR LF, no final newline, blank lines, a header line among records."""
    w = tiny_case()
    lines = []
    for i in range(len(w.records)):
        r = int(w.records.ref_id[i])
        lines.append(f"r{int(w.records.read_key[i])}\t{int(w.records.flag[i])}\t{w.ref_names[r] if r >= 0 else '*'}\t"
                     f"{int(w.records.begin_pos[i]) + 1}\t255\t50M\t*\t0\t0\t{'A' * 50}\t*")
    head = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{int(l)}\n" for n, l in zip(w.ref_names, w.ref_len))
    body = "\n".join(lines) + "\n"
    return {
        "crlf": (head + body).replace("\n", "\r\n"),
        "no_final_newline": head + body[:-1],
        "crlf_no_final_newline": (head + body).replace("\n", "\r\n")[:-2],
        "blank_lines": head + "\n" + "\n".join(lines[:3]) + "\n\n" + "\n".join(lines[3:]) + "\n\n",
        "header_among_records": head + "\n".join(lines[:4]) + "\n@CO\tlate\n" + "\n".join(lines[4:]) + "\n",
        "short_line": head + "\n".join(lines[:4]) + "\nr1\t0\t*\n" + "\n".join(lines[4:]) + "\n",
        "only_header_no_newline": head[:-1],
        "empty": "",
    }


@pytest.mark.parametrize("name", sorted(odd_texts()))
def test_odd_text_reads_as_in_the_plain_file(tmp_path, name):
    text = odd_texts()[name].encode()
    p = str(tmp_path / "x.sam")
    open(p, "wb").write(text)
    plain = run(["--dump-records", p])
    for kind, blob in (("bgzf", bgzf(text, seed=2, lo=1, hi=97)), ("gzip", gzip_members(text, 2))):
        q = str(tmp_path / f"x.{kind}.sam.gz")
        open(q, "wb").write(blob)
        got = run(["--dump-records", q])
        assert (got.returncode, got.stdout, got.stderr) == (plain.returncode, plain.stdout, plain.stderr), kind
