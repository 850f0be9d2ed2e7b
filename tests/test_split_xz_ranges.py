"""slimm_host_xz_ranges and slimm_host_xz_check_at (host only): the byte ranges of an xz-compressed SAM file that the members
of a group read with --split-input, planned from the file's index or indexes alone.  A cut is the first byte of a block that
is not the first of its stream, the first byte of a stream header, or the file's size; the ranges cover the file once; no cut
lies in front of the end of the block that holds the SAM header's last byte; cut i is the earliest legal cut at or behind
first + i * (size - first) / n.  The inputs: the committed files of tests/golden/xz and containers written in Python
(tests/sam_xz.py); what they hold is stated by the tests' own walker, X.walk.  No GPU is touched."""
import ctypes as C
import os
import subprocess

import pytest

from slimm_amd import capi
from tests import sam_xz as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(X.GOLDEN_KINDS)
WRITTEN = ["stored_chunks", "reblocked", "two_streams_padded", "empty_stream"]


def ranges(path, n, skip=0, want=capi.OK):
    out = (C.c_uint64 * (n + 1))()
    assert capi.lib().slimm_host_xz_ranges(str(path).encode(), skip, n, out) == want
    return list(out)


def check_at(path, offset, want=capi.OK):
    kind = C.c_int(-2)
    assert capi.lib().slimm_host_xz_check_at(str(path).encode(), offset, C.byref(kind)) == want
    return kind.value


def legal_cuts(blob):
    """where a file may be cut, by the walker: every stream header, every block but a stream's first, the file's size"""
    out = []
    for s in X.walk(blob):
        out.append(s["at"])
        out += [b["at"] for b in s["blocks"][1:]]
    return out + [len(blob)]


def first_cut(blob, skip):
    """the end of the block that holds decoded byte skip - 1 (its padding and check included); 0 without a header"""
    text = 0
    for s in X.walk(blob):
        for b in s["blocks"]:
            text += b["text"]
            if skip and text >= skip:
                return b["check_at"] + X.CHECK_BYTES[s["check"]]
    assert not skip
    return 0


def planned(blob, skip, n):
    """the plan, from the rule"""
    cuts, first, size = legal_cuts(blob), first_cut(blob, skip), len(blob)
    return [0] + [min(c for c in cuts if c >= first + i * (size - first) // n) for i in range(1, n)] + [size]


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("texts")
    return {(g, n): X.case_text(d, g, n) for g in (True, False) for n in (1_000, 3_000, 15_000)}


def blob_of(texts, kind, grouped=True):
    tag = "grouped" if grouped else "any"
    if kind in X.GOLDEN_KINDS:
        n, name = X.GOLDEN_KINDS[kind]
        return texts[(grouped, n)], X.golden(name.format(tag))
    text = texts[(grouped, 1_000)]
    return text, X.written_copies(text, tag)[kind]


def small_blocks(text, blocks=10, check=4):
    """4 000 bytes of the text in stored blocks of 400: the header (476 bytes) spans the first two"""
    return X.stored_chunks(text[:4_000], step=300, check=check, blocks=blocks)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind", GOLDEN + WRITTEN)
def test_every_cut_is_the_earliest_legal_one_behind_its_target(tmp_path, texts, kind, grouped):
    text, blob = blob_of(texts, kind, grouped)
    p = tmp_path / "x.sam.xz"
    p.write_bytes(blob)
    cuts = set(legal_cuts(blob))
    for skip in (0, X.header_len(text)):
        for n in (1, 2, 3, 4, 5):
            offs = ranges(p, n, skip)
            assert offs[0] == 0 and offs[n] == len(blob)
            assert all(a <= b for a, b in zip(offs, offs[1:]))
            assert all(o in cuts for o in offs[1:]), (offs, sorted(cuts))
            assert offs == planned(blob, skip, n), (kind, skip, n)
            if skip:
                assert all(o >= first_cut(blob, skip) > 0 for o in offs[1:])
    if kind == "mt":   # (14 blocks with sizes in their headers: enough for every member)
        assert len(X.walk(blob)[0]["blocks"]) == 14 and len(set(ranges(p, 5, X.header_len(text)))) == 6


def test_a_header_over_two_blocks_puts_the_first_cut_behind_the_second(tmp_path, texts):
    text = texts[(True, 1_000)]
    skip = X.header_len(text)
    blob = small_blocks(text)
    blocks = X.walk(blob)[0]["blocks"]
    assert len(blocks) == 10 and blocks[0]["text"] == 400 < skip < 800
    p = tmp_path / "x.sam.xz"
    p.write_bytes(blob)
    for n in (2, 5, 64):
        assert min(ranges(p, n, skip)[1:]) >= blocks[2]["at"]
        assert min(ranges(p, n, 150)[1:]) >= blocks[1]["at"]
    many = len(blob) + 1   # (more members than bytes: the first target is the first legal cut itself)
    assert ranges(p, many, skip)[1] == blocks[2]["at"]
    assert ranges(p, many, 150)[1] == blocks[1]["at"]
    assert ranges(p, many, 400)[1] == blocks[1]["at"]      # (decoded byte 399 is the first block's last)
    assert ranges(p, many, 401)[1] == blocks[2]["at"]
    assert ranges(p, many, 0)[1] == 0
    assert ranges(p, many, 4_000)[1] == len(blob)           # (the last block holds it: no cut is left but the file's size)


def test_the_cut_in_front_of_a_second_stream_is_its_header(tmp_path, texts):
    """Two streams with padding behind each: stream 2's first block is no cut, its header is, and the padding in front of it
    stays on the left."""
    text, blob = blob_of(texts, "two_streams_padded")
    one, two = X.walk(blob)
    assert one["padding"] == 8 and two["padding"] == 4 and len(one["blocks"]) == 1 and len(two["blocks"]) == 2
    p = tmp_path / "x.sam.xz"
    p.write_bytes(blob)
    assert two["blocks"][0]["at"] not in legal_cuts(blob)
    for n in (2, 3):
        assert ranges(p, n, X.header_len(text)) == planned(blob, X.header_len(text), n)
    many = ranges(p, len(blob) + 1, X.header_len(text))
    assert many[1] == two["at"] == one["end"] + 8      # (the header's block is stream 1's last: the index behind it is no cut)
    assert set(many) == {0, two["at"], two["blocks"][1]["at"], len(blob)}
    # an empty stream in front: its header and the next stream's are cuts
    text, blob = blob_of(texts, "empty_stream")
    p.write_bytes(blob)
    empty, real = X.walk(blob)
    assert not empty["blocks"] and set(ranges(p, len(blob) + 1, 0)) == {0, real["at"]} | {b["at"] for b in real["blocks"][1:]} | {len(blob)}


def test_more_members_than_blocks_gives_empty_ranges(tmp_path, texts):
    text, blob = blob_of(texts, "reblocked")
    assert len(X.walk(blob)[0]["blocks"]) == 3
    p = tmp_path / "x.sam.xz"
    p.write_bytes(blob)
    offs = ranges(p, 8, X.header_len(text))
    assert offs == planned(blob, X.header_len(text), 8)
    assert sum(1 for a, b in zip(offs, offs[1:]) if a == b) >= 5   # (the header's block is member 0's: two cuts are left at most)
    text, blob = blob_of(texts, "one")
    p.write_bytes(blob)
    for n in (2, 4):
        assert ranges(p, n, X.header_len(text)) == [0] + [len(blob)] * n   # (one block: member 0 reads it)


@pytest.mark.parametrize("check", [0, 1, 4, 10])
def test_the_check_kind_at_an_offset(tmp_path, texts, check):
    """-1 at 0 and at stream headers (a range that starts there reads the kind itself), the stream's kind at its blocks."""
    text = texts[(True, 1_000)]
    parts = X.part_blocks(text, "grouped")
    other = 4 if check != 4 else 1
    blob = X.stream_of(parts, check=check) + bytes(8) + X.stream_of(parts[:2], check=other)
    p = tmp_path / "x.sam.xz"
    p.write_bytes(blob)
    one, two = X.walk(blob)
    assert (one["check"], two["check"]) == (check, other)
    assert check_at(p, 0) == -1 and check_at(p, two["at"]) == -1 and check_at(p, len(blob)) == -1
    assert check_at(p, one["end"] + 4) == -1                    # (stream padding)
    assert [check_at(p, b["at"]) for b in one["blocks"][1:]] == [check] * 2
    assert [check_at(p, b["at"]) for b in two["blocks"][1:]] == [other]
    assert check_at(p, one["blocks"][1]["at"] + 4) == check      # (any byte of the stream)
    for offs in (ranges(p, 3, X.header_len(text)), ranges(p, 5, 0)):
        for o in offs[:-1]:
            assert check_at(p, o) == (-1 if o in (0, two["at"], len(blob)) else check if o < one["end"] else other)


def test_what_cannot_be_planned(tmp_path, texts):
    text, blob = blob_of(texts, "mt")
    p = tmp_path / "x.sam.xz"
    p.write_bytes(blob)
    ranges(p, 2, len(text))
    ranges(p, 2, len(text) + 1, want=capi.E_INVALID)           # (a skip beyond the text the index states)
    ranges(p, 2, 1 << 32, want=capi.E_INVALID)
    ranges(tmp_path, 2, 0, want=capi.E_INVALID)                # (a directory)
    ranges(tmp_path / "missing.xz", 2, 0, want=capi.E_INVALID)
    check_at(tmp_path / "missing.xz", 0, want=capi.E_INVALID)
    fifo = tmp_path / "pipe.sam.xz"
    os.mkfifo(fifo)
    ranges(fifo, 2, 0, want=capi.E_INVALID)
    check_at(fifo, 0, want=capi.E_INVALID)
    q = tmp_path / "cut.sam.xz"
    s = X.walk(blob)[0]
    for end in (len(blob) - 4, s["footer_at"], s["index_at"] + 8, s["index_at"]):   # (a truncated footer, a truncated index, none)
        q.write_bytes(blob[:end])
        ranges(q, 2, 0, want=capi.E_INVALID)
        check_at(q, 100, want=capi.E_INVALID)
    bad = bytearray(blob)
    bad[s["index_at"] + 3] ^= 1                                 # (an index whose CRC32 does not hold)
    q.write_bytes(bytes(bad))
    ranges(q, 2, 0, want=capi.E_INVALID)
    q.write_bytes(text)
    ranges(q, 2, 10, want=capi.E_INVALID)                      # (no xz file)
    q.write_bytes(b"")
    ranges(q, 2, 0, want=capi.E_INVALID)


def test_the_floor_is_sixteen_blocks_unless_forced(monkeypatch):
    """... by a key of its own: xz_device_blocks decides whether the device reads the file at all, and does not move it."""
    L = capi.lib()
    monkeypatch.delenv("SLIMM_FORCE", raising=False)
    assert L.slimm_xz_split_floor() == 16
    monkeypatch.setenv("SLIMM_FORCE", "xz_device_blocks=3")
    assert L.slimm_xz_split_floor() == 16
    monkeypatch.setenv("SLIMM_FORCE", "xz_device_blocks=3,xz_split_blocks=2")
    assert L.slimm_xz_split_floor() == 2
    monkeypatch.setenv("SLIMM_FORCE", "xz_split_blocks=0")
    assert L.slimm_xz_split_floor() == 0


def test_the_sanitizer_program_ends_clean(tmp_path, texts):
    """tests/native/san_xz_ranges.cpp under AddressSanitizer and UBSan (a stand-alone program: nothing is loaded here): the
    planner and the check lookup over every committed input and the written containers -- whole, truncated at every 4-byte
    step of their last 256 bytes, and with bit flips there.  Damage ends in "no plan", never in a report."""
    exe = str(tmp_path / "san_xz_ranges")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_xz_ranges.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", "xz.cpp"),
                    "-o", exe], check=True)
    paths = [os.path.join(X.GOLDEN, f) for f in sorted(os.listdir(X.GOLDEN)) if f.endswith(".xz")]
    text = texts[(True, 1_000)]
    written = dict(X.written_copies(text, "grouped"), small_blocks=small_blocks(text))
    for name, blob in written.items():
        (tmp_path / (name + ".xz")).write_bytes(blob)
        paths.append(str(tmp_path / (name + ".xz")))
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == len(paths), r.stdout
    for line in lines:   # (whole: 6 member counts x skips 0, 1 and 476 are planned, 2^40 is refused)
        assert "whole: 18 plans, 6 refused" in line, line
    golden_lines = [l for l in lines if "config1_" in l or "long_" in l]   # (no stream padding: every truncated copy is refused)
    assert len(golden_lines) == 6 and all("truncated: 0 plans, 1280 refused" in l for l in golden_lines), golden_lines
