"""slimm_host_zstd_ranges (host only): the byte ranges of a zstd-compressed SAM file that the members of a group read with
--split-input.  A cut is the first byte of a frame or of a skippable frame, or the file's size; the ranges cover the file
once; no cut lies in front of the end of the frame that holds the SAM header's last byte; a look-alike inside a block's
content is no cut; the search for a cut is bounded.  The committed inputs of tests/golden/zstd_frames are checked against
their texts, made again from their seeds, through the product's host decoder.  No GPU is touched."""
import ctypes as C
import os
import subprocess

import pytest

from slimm_amd import capi
from tests import sam_zst as Z
from tests.sam_gz import header_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = os.path.join(ROOT, "tests", "golden", "zstd_frames")
GOLDEN = [f"config1_{tag}_frames_l{level}.sam.zst" for tag in ("grouped", "any") for level in (3, 19)]


def golden(name):
    return open(os.path.join(FRAMES, name), "rb").read()


def ranges(path, n, skip=0, want=capi.OK):
    out = (C.c_uint64 * (n + 1))()
    assert capi.lib().slimm_host_zstd_ranges(str(path).encode(), skip, n, out) == want
    return list(out)


def starts(blob):
    """where a file may be cut: the first byte of every frame and skippable frame (Z.walk), and its size"""
    return {f["at"] for f in Z.walk(blob)} | {len(blob)}


def frame_ends(blob):
    at = sorted(starts(blob))
    return at[1:]


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("texts")
    return {g: Z.case_text(d, g, 3_000) for g in (True, False)}


def raw_frames(text, step=30_000, extras=True):
    """frames of `step` bytes of text in raw blocks, with an empty frame and a skippable frame between them"""
    out = []
    for i in range(0, len(text), step):
        out.append(Z.raw_frame(text[i:i + step], step=step, checksum=i % (2 * step) == 0))
        if extras and i // step == 1:
            out.append(Z.raw_frame(b""))
        if extras and i // step in (0, 2):
            out.append(Z.skippable())
    return b"".join(out)


def test_the_committed_files_decode_to_their_texts(tmp_path, texts):
    exe = str(tmp_path / "san_zstd")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "native", "san_zstd.cpp"),
                    os.path.join(ROOT, "slimm_amd", "csrc", "host", "zstd.cpp"), "-o", exe], check=True)
    assert len(texts[True]) == 445_770 and header_len(texts[True]) == 476
    assert len(golden(GOLDEN[0])) == 27_582
    for name in GOLDEN:
        blob = golden(name)
        c = Z.census(blob)
        assert (c["frames"], c["skippable"]) == (7, 7), (name, c)
        assert all(f["skippable"] == (i % 2 == 0) for i, f in enumerate(Z.walk(blob)))   # (pzstd: one in front of every frame)
        out = str(tmp_path / "out.bin")
        subprocess.run([exe, "--out", out, os.path.join(FRAMES, name)], check=True)
        assert open(out, "rb").read() == texts["grouped" in name], name


@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 64])
@pytest.mark.parametrize("kind", ["golden_l3", "golden_l19", "raw30k", "written"])
def test_every_cut_is_a_frame_start(tmp_path, texts, kind, n):
    text = texts[True]
    blob = {"golden_l3": lambda: golden(GOLDEN[0]), "golden_l19": lambda: golden(GOLDEN[1]), "raw30k": lambda: raw_frames(text),
            "written": lambda: Z.written_copies(text)["frames"]}[kind]()
    p = tmp_path / "x.sam.zst"
    p.write_bytes(blob)
    at = starts(blob)
    for skip in (0, header_len(text)):
        offs = ranges(p, n, skip)
        assert offs[0] == 0 and offs[n] == len(blob)
        assert all(a <= b for a, b in zip(offs, offs[1:]))
        assert all(o in at for o in offs[1:]), (offs, sorted(at))
        if skip:   # (member 0 holds the header's frame: the first content frame's end)
            first = [f for f in Z.walk(blob) if not f["skippable"]][0]["at"]
            assert all(o > first for o in offs[1:])
    if n in (2, 4) and kind != "written":
        assert len(set(ranges(p, n, header_len(text)))) == n + 1   # (enough frames: no range is empty)


def test_a_header_over_two_frames_puts_the_first_cut_behind_the_second(tmp_path, texts):
    text = texts[True]
    skip = header_len(text)
    text = text[:4_000]   # (small: the test plans for more members than the file has bytes)
    pieces = [text[:200], text[200:1_000]] + [text[i:i + 1_000] for i in range(1_000, len(text), 1_000)]
    assert 200 < skip < 1_000
    blob = b"".join(Z.raw_frame(p) for p in pieces)
    p = tmp_path / "x.sam.zst"
    p.write_bytes(blob)
    ends = frame_ends(blob)
    for n in (2, 5, 64):
        assert min(ranges(p, n, skip)[1:]) >= ends[1]
        assert min(ranges(p, n, 150)[1:]) >= ends[0]
    many = len(blob) + 1   # (more members than bytes: the first target is the first legal cut itself)
    assert ranges(p, many, skip)[1] == ends[1]
    assert ranges(p, many, 150)[1] == ends[0]
    assert ranges(p, many, 200)[1] == ends[0]       # (decoded byte 199 is the first frame's last)
    assert ranges(p, many, 201)[1] == ends[1]
    assert ranges(p, many, 0)[1] == 0


def test_one_frame_gives_cuts_at_the_files_size(tmp_path, texts):
    for blob in (Z.golden("config1_grouped_l19.sam.zst"), Z.raw_frame(texts[True])):
        p = tmp_path / "x.sam.zst"
        p.write_bytes(blob)
        for n in (2, 4):
            for skip in (0, header_len(texts[True])):
                assert ranges(p, n, skip) == [0] + [len(blob)] * n


def test_a_target_on_a_frame_start_takes_it(tmp_path, texts):
    a, b = Z.raw_frame(texts[True][:30_000]), Z.raw_frame(texts[True][30_000:60_000])
    assert len(a) == len(b)
    p = tmp_path / "x.sam.zst"
    p.write_bytes(a + b)
    assert ranges(p, 2, 0) == [0, len(a), 2 * len(a)]
    p.write_bytes(a + b + a + b)
    assert ranges(p, 4, 0) == [i * len(a) for i in range(5)]


def test_magic_bytes_in_a_raw_block_are_no_cut(tmp_path, texts):
    """The 4 magic bytes followed by text, all over a raw block's content: the header behind them does not parse, or its
    block chain does not hold."""
    head = Z.raw_frame(texts[True][:1000])
    body = (Z.MAGIC + b"\tr1\t0\tref\t100\n") * 4000
    tail = Z.raw_frame(texts[True][1000:3000])
    blob = head + Z.raw_frame(body) + tail
    p = tmp_path / "x.sam.zst"
    p.write_bytes(blob)
    at = starts(blob)
    assert blob.count(Z.MAGIC) >= 4003
    for n in (2, 3, 7, 50):
        offs = ranges(p, n)
        assert all(o in at for o in offs), offs
    assert ranges(p, 2)[1] == len(blob) - len(tail)


def test_a_whole_look_alike_frame_in_a_raw_block_is_no_cut(tmp_path, texts):
    """Magic, a header that parses (single segment, 5 bytes of content), a last raw block of 5 bytes -- and behind it neither
    a magic nor the file's end: no cut.  The same bytes as a real frame in front of the next frame are one."""
    fake = Z.frame_header(5, False, None) + Z.block(0, b"hello", last=True)
    assert len(Z.walk(fake)) == 1
    head = Z.raw_frame(texts[True][:1000])
    body = (fake + b"zzzz\n") * 3000
    tail = Z.raw_frame(texts[True][1000:3000])
    blob = head + Z.raw_frame(body) + tail
    p = tmp_path / "x.sam.zst"
    p.write_bytes(blob)
    at = starts(blob)
    for n in (2, 3, 7, 50):
        assert all(o in at for o in ranges(p, n))
    assert ranges(p, 2)[1] == len(blob) - len(tail)
    real = head + fake + tail
    p.write_bytes(real)
    assert set(ranges(p, 50)) == starts(real)


def test_the_search_for_a_cut_is_bounded(tmp_path, texts, monkeypatch):
    """SLIMM_FORCE zstd_cut_search=1000 over frames of 50 000 bytes: no start within 1 000 bytes of a target, so every cut
    is the file's size and the ranges behind member 0's are empty."""
    text = texts[True]
    blob = b"".join(Z.raw_frame(text[i:i + 50_000], step=50_000) for i in range(0, 200_000, 50_000))
    p = tmp_path / "x.sam.zst"
    p.write_bytes(blob)
    skip = header_len(text)
    at = sorted(starts(blob))
    assert ranges(p, 4, skip) == [0, at[2], at[3], at[4], at[4]]   # (targets inside frames 2, 3 and 4: the next starts)
    monkeypatch.setenv("SLIMM_FORCE", "zstd_cut_search=1000")
    assert ranges(p, 4, skip) == [0] + [len(blob)] * 4
    monkeypatch.setenv("SLIMM_FORCE", "zstd_cut_search=13000")      # (12 505 bytes from target 1 to frame 3: found; the others not)
    assert ranges(p, 4, skip) == [0, at[2], len(blob), len(blob), len(blob)]


def test_what_cannot_be_planned(tmp_path, texts):
    text = texts[True]
    blob = raw_frames(text)
    p = tmp_path / "x.sam.zst"
    p.write_bytes(blob)
    ranges(p, 2, len(text))
    ranges(p, 2, len(text) + 1, want=capi.E_INVALID)           # (a skip beyond the text)
    ranges(p, 2, 1 << 32, want=capi.E_INVALID)
    ranges(tmp_path, 2, 0, want=capi.E_INVALID)                # (a directory)
    ranges(tmp_path / "missing.zst", 2, 0, want=capi.E_INVALID)
    fifo = tmp_path / "pipe.sam.zst"
    os.mkfifo(fifo)
    ranges(fifo, 2, 0, want=capi.E_INVALID)
    q = tmp_path / "x.sam"
    q.write_bytes(text)
    ranges(q, 2, 10, want=capi.E_INVALID)                      # (no zstd frame: the header's frames do not decode)


def test_the_floor_is_the_round_size_unless_forced(monkeypatch):
    L = capi.lib()
    monkeypatch.delenv("SLIMM_FORCE", raising=False)
    assert L.slimm_zstd_split_floor() == 32 << 20
    monkeypatch.setenv("SLIMM_FORCE", "zstd_split_floor=0")
    assert L.slimm_zstd_split_floor() == 0
    monkeypatch.setenv("SLIMM_FORCE", "zstd_round=5,zstd_split_floor=4096")
    assert L.slimm_zstd_split_floor() == 4096


def test_the_sanitizer_program_ends_clean(tmp_path, texts):
    """tests/native/san_zstd_ranges.cpp under AddressSanitizer and UBSan (a stand-alone program: nothing is loaded here): the
    candidate test and the chain walk over two small written blobs -- whole, at every prefix length, with 2 000 bit flips
    each.  Damage ends in "no cut", never in a report.  (The committed files take a minute: the program's header says how.)"""
    exe = str(tmp_path / "san_zstd_ranges")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_zstd_ranges.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", "zstd.cpp"),
                    "-o", exe], check=True)
    text = texts[True]
    fake = Z.frame_header(5, False, None) + Z.block(0, b"hello", last=True)
    blobs = {
        "lookalike.zst": Z.raw_frame(text[:600]) + Z.raw_frame((fake + b"zzzz\n") * 60) + Z.skippable() + Z.raw_frame(text[600:1500], rle=True),
        "magics.zst": Z.raw_frame(text[:600], checksum=False) + Z.raw_frame((Z.MAGIC + b"\tr1\t0\tref\n") * 80) + Z.raw_frame(b"") + Z.raw_frame(text[600:900]),
    }
    paths = []
    for name, blob in blobs.items():
        (tmp_path / name).write_bytes(blob)
        paths.append(str(tmp_path / name))
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 2, r.stdout
    for line, blob in zip(lines, blobs.values()):   # (every frame and skippable frame start of the whole blob is a cut, nothing else)
        assert f"whole: {len(Z.walk(blob))} cuts of {len(blob)} candidates" in line, line
