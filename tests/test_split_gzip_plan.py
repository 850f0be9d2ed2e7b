"""slimm_host_gzip_ranges (host only): the BIT ranges of a gzip-compressed SAM file that the members of a group read with
--split-input (include/slimm_hip.h, "gzip SAM by byte range").  A cut is the first bit of a non-final dynamic block, or 8 x
the file's size; the ranges cover the file once; no cut lies in front of the end of the block that holds the SAM header's
last byte; a stream of stored or fixed blocks only is not cut; a block header with nothing valid behind it is no cut.  What
a file's blocks are is said by the pure-Python walker of tests/sam_deflate.py.  The planner's core (slimm_amd/csrc/gzip_plan.h)
also runs under AddressSanitizer and UBSan as a stand-alone program.  No GPU is touched."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from slimm_amd import capi
from slimm_amd.synth import CONFIGS, make_workload
from tests import sam_deflate as D
from tests.bam_io import write_sam
from tests.test_gpu_bam_decode import _named

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = list(D.KINDS) + ["members"]


def ranges(path, n, skip=0, want=capi.OK):
    out = (C.c_uint64 * (n + 1))()
    assert capi.lib().slimm_host_gzip_ranges(str(path).encode(), skip, n, out) == want
    return list(out)


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    w = _named(make_workload(CONFIGS["config1"], seed=41, n_records=4000))
    p = str(tmp_path_factory.mktemp("text") / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    return open(p, "rb").read()


def file_blocks(blob):
    """Every deflate block of a gzip file of several members: [(the FILE's bit, type, final, text bytes, text bytes in front)]"""
    out, at, before = [], 0, 0
    while at < len(blob):
        h = 10
        flg = blob[at + 3]
        if flg & 4:
            h += 2 + struct.unpack_from("<H", blob, at + h)[0]
        for f in (8, 16):
            if flg & f:
                h = blob.index(b"\0", at + h) - at + 1
        if flg & 2:
            h += 2
        bl, end = D.blocks(blob, (at + h) * 8)
        for bit, typ, final, n in bl:
            out.append((bit, typ, final, n, before))
            before += n
        at = (end + 7) // 8 + 8
    return out


def check_plan(blob, offs, n, skip):
    bl = file_blocks(blob)
    cuts_ok = {b[0] for b in bl if b[1] == 2 and not b[2]}
    assert offs[0] == 0 and offs[n] == 8 * len(blob)
    assert all(a <= b for a, b in zip(offs, offs[1:]))
    interior = [o for o in offs[1:n] if o < 8 * len(blob)]
    assert all(o in cuts_ok for o in interior), (interior, sorted(cuts_ok)[:10])
    # the floor: the end of the block that holds text byte skip - 1 is the start of the next block (or lies in a trailer)
    if skip:
        holder = next(i for i, b in enumerate(bl) if b[4] + b[3] >= skip)
        assert all(o > bl[holder][0] for o in interior)
    return interior


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_every_cut_is_the_start_of_a_non_final_dynamic_block(tmp_path, text, kind, n):
    blob = D.copy_of(text, kind)
    p = tmp_path / "x.sam.gz"
    p.write_bytes(blob)
    dynamic = sum(1 for b in file_blocks(blob) if b[1] == 2 and not b[2])
    for skip in (0, D.header_len(text)):
        offs = ranges(p, n, skip)
        interior = check_plan(blob, offs, n, skip)
        if kind in ("stored", "fixed"):
            assert offs == [0] + [8 * len(blob)] * n       # (no dynamic block: nothing to cut at)
        if kind in ("mem1", "mem3", "rle", "sync") and n <= 4:
            assert dynamic >= 20                           # (said by the walker: enough blocks that ...)
            assert len(set(offs)) == n + 1, offs           # (... no range is empty)
        if kind == "default":
            assert dynamic <= 2 and len(interior) <= dynamic   # (a block or two: most members stay empty)


def test_a_second_copy_at_another_memlevel(tmp_path, text):
    """A mem1 copy of 120 000 bytes of the text: cuts at other bits, the same rules; the ranges' bytes share at most one."""
    blob = D.member(text[:120_000], memLevel=1)
    p = tmp_path / "x.sam.gz"
    p.write_bytes(blob)
    for n in (2, 4, 8):
        offs = ranges(p, n, D.header_len(text))
        check_plan(blob, offs, n, D.header_len(text))
        for a, b in zip(offs, offs[1:]):
            assert (a + 7) // 8 - a // 8 <= 1 and b // 8 <= len(blob)


def test_the_floor_follows_the_skip(tmp_path, text):
    """More members than the file has bits: the first target is the floor itself, and the first cut the first block behind
    the one that holds byte skip - 1."""
    small = text[:20_000]
    blob = D.member(small, memLevel=1)
    p = tmp_path / "x.sam.gz"
    p.write_bytes(blob)
    bl = file_blocks(blob)
    assert len(bl) >= 8 and all(b[1] == 2 for b in bl)
    many = 8 * len(blob) + 1
    assert ranges(p, many, 0)[1] == bl[0][0] == 80                   # (skip 0: a cut right behind the member header)
    for k in (1, 3, 5):
        skip = bl[k][4] + 1                                            # (byte skip - 1 is block k's first)
        assert ranges(p, many, skip)[1] == bl[k + 1][0]
        assert ranges(p, many, skip - 1)[1] == bl[k][0]                # (... block k - 1's last)
    assert ranges(p, 2, len(small))[1] == 8 * len(blob)                # (all of the text is header: the final block's end)
    ranges(p, 2, len(small) + 1, want=capi.E_INVALID)                  # (the text ends in front of that byte)


def stored_block(payload: bytes, final=False) -> bytes:
    return bytes([1 if final else 0]) + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload


def test_a_block_header_in_a_stored_block_with_nothing_behind_it_is_no_cut(tmp_path, text):
    """The first 90 bytes of a real dynamic block -- its whole header: gz::is_candidate holds -- in a stored block's bytes,
    0xff behind it to the stored block's end: the walk from there finds no chain of blocks.  The real dynamic blocks behind
    the stored block are cuts."""
    real = D.member(text[:60_000], memLevel=1)
    bl = D.member_blocks(real)
    k = next(i for i, b in enumerate(bl) if b[1] == 2 and not b[2] and b[0] % 8 == 0 and i > 0)   # (byte-aligned: it can be pasted)
    head = real[10 + bl[k][0] // 8:][:90]
    payload = text[1_000:9_000] + head + b"\xff" * 20_000
    tail = D.raw_deflate(text[60_000:120_000], memLevel=1)
    deflate = stored_block(text[:1_000]) + stored_block(payload) + tail
    whole = text[:1_000] + payload + text[60_000:120_000]
    blob = D.gzip_frame(deflate, whole)
    import zlib
    assert zlib.decompress(blob, 31) == whole
    p = tmp_path / "x.sam.gz"
    p.write_bytes(blob)
    first_real = 8 * (10 + len(deflate) - len(tail))
    for n in (2, 3, 7):
        offs = ranges(p, n)
        check_plan(blob, offs, n, 0)
        assert all(o >= first_real for o in offs[1:]), (offs, first_real)
    # the same header with nothing at all behind it: the bytes run out before a boundary is passed
    blob2 = D.gzip_frame(stored_block(text[:1_000]) + stored_block(head, final=True), text[:1_000] + head)
    p.write_bytes(blob2)
    assert ranges(p, 2) == [0, 8 * len(blob2), 8 * len(blob2)]


def test_the_search_and_the_walk_are_bounded(tmp_path, text, monkeypatch):
    blob = D.member(text, memLevel=1)
    p = tmp_path / "x.sam.gz"
    p.write_bytes(blob)
    skip = D.header_len(text)
    usual = ranges(p, 4, skip)
    assert len(set(usual)) == 5
    monkeypatch.setenv("SLIMM_FORCE", "gzip_cut_search=1")        # (one byte behind each target: hardly a block start)
    offs = ranges(p, 4, skip)
    check_plan(blob, offs, 4, skip)
    assert len(set(offs)) < 5
    monkeypatch.setenv("SLIMM_FORCE", "gzip_cut_blocks=1")        # (one boundary is enough: the same cuts on a real file)
    assert ranges(p, 4, skip) == usual
    monkeypatch.setenv("SLIMM_FORCE", "gzip_cut_blocks=100000")   # (more boundaries than blocks: the final block ends the walk)
    assert ranges(p, 4, skip) == usual
    monkeypatch.setenv("SLIMM_FORCE", "gzip_split_wrong_cut")
    wrong = ranges(p, 4, skip)
    assert wrong[2] == usual[2] + 1 and wrong[:2] + wrong[3:] == usual[:2] + usual[3:]


def test_what_cannot_be_planned(tmp_path, text):
    blob = D.member(text, memLevel=1)
    p = tmp_path / "x.sam.gz"
    p.write_bytes(blob)
    ranges(p, 2, 1 << 32, want=capi.E_INVALID)
    ranges(tmp_path, 2, 0, want=capi.E_INVALID)                   # (a directory)
    ranges(tmp_path / "missing.gz", 2, 0, want=capi.E_INVALID)
    fifo = tmp_path / "pipe.sam.gz"
    os.mkfifo(fifo)
    ranges(fifo, 2, 0, want=capi.E_INVALID)
    q = tmp_path / "x.sam"
    q.write_bytes(text)
    ranges(q, 2, 10, want=capi.E_INVALID)                         # (no gzip member)
    bad = bytearray(blob)
    bad[10] |= 0x06                                               # (the first block's type: 3)
    q.write_bytes(bytes(bad))
    ranges(q, 2, 10, want=capi.E_INVALID)                         # (a header that does not inflate)
    q.write_bytes(blob[:200])
    ranges(q, 2, D.header_len(text), want=capi.E_INVALID)         # (... or ends in front of its last byte)


def test_the_floor_of_the_command_and_todays_file(tmp_path, monkeypatch):
    """slimm_gzip_split_floor is 32 MiB unless told.  The two-member file of tests/test_cli_split_input_sam.py's gzip test --
    config 1, 20 000 records -- is far below it for four members: that test keeps its path and its trace line."""
    L = capi.lib()
    monkeypatch.delenv("SLIMM_FORCE", raising=False)
    assert L.slimm_gzip_split_floor() == 32 << 20
    w = make_workload(CONFIGS["config1"], seed=3)
    p = str(tmp_path / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    whole = open(p, "rb").read()
    import gzip
    half = len(whole) // 2
    blob = gzip.compress(whole[:half]) + gzip.compress(whole[half:])
    assert len(blob) // 4 < (32 << 20) // 8                        # (eight times too small, whatever the first cut)
    monkeypatch.setenv("SLIMM_FORCE", "gzip_split_floor=0")
    assert L.slimm_gzip_split_floor() == 0
    monkeypatch.setenv("SLIMM_FORCE", "gzip_round=5,gzip_split_floor=4096")
    assert L.slimm_gzip_split_floor() == 4096


def test_the_sanitizer_program_ends_clean(tmp_path, text):
    """tests/native/san_gzip_plan.cpp under AddressSanitizer and UBSan (a stand-alone program: nothing is loaded here): the
    plan of each file for 2, 4 and 8 members with and without a skip, of every prefix in steps, and of copies with flipped
    bits.  Damage ends in "not planned" or in other cuts, never in a report."""
    exe = str(tmp_path / "san_gzip_plan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_gzip_plan.cpp"), "-o", exe], check=True)
    small = text[:40_000]
    blobs = {"mem1.gz": D.member(small, memLevel=1), "members.gz": D.three_members(small), "stored.gz": D.member(small, level=0)}
    paths = []
    for name, blob in blobs.items():
        (tmp_path / name).write_bytes(blob)
        paths.append(str(tmp_path / name))
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 3, r.stdout
    for line, (name, blob) in zip(lines, blobs.items()):
        p = tmp_path / name
        want = " ".join(str(v) for v in ranges(p, 4, 0))
        assert f"whole: {want};" in line, (line, want)            # (the program's plan is the library's)
