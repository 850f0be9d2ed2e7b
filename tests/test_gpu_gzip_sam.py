"""gzip-compressed SAM on a real MI355X: slimm_push_gzip_sam_bytes (the file's bytes, cut anywhere; chunk starts found, the
chunks inflated in parallel, what they copy from the chunk in front resolved, every member checked on the device, the text
found and decoded as SAM) against slimm_push_sam_bytes on the same text and the CPU oracle.  slimm_get_gzip_stats says
that an input reached what it was built for.  The inputs: tests/sam_deflate.py."""
import ctypes as C
import os
import random
import zlib

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from slimm_amd.synth import CONFIGS, make_workload
from tests import sam_deflate as D
from tests.helpers import assert_matches_oracle
from tests.test_gpu_bam_decode import _named
from tests.test_gpu_compressed_sam import integers, profile_of, sam_text

pytestmark = pytest.mark.gpu

SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)
CORRUPT, TRUNCATED = "corrupt gzip stream (", "truncated gzip stream"
KINDS = ["default", "mem1", "fixed", "rle", "sync", "stored", "members"]


def forced(monkeypatch, value):
    if value:
        monkeypatch.setenv("SLIMM_FORCE", value)
    else:
        monkeypatch.delenv("SLIMM_FORCE", raising=False)


def random_cuts(n, seed, lo, hi):
    rng, p, out = random.Random(seed), 0, []
    while True:
        p += rng.randint(lo, hi)
        if p >= n:
            return out
        out.append(p)


_shared = {}


def case(tmp_path, grouped, tail_newline=True):
    """The 3 000-record text, its header's length, the oracle's run and the profile of the plain text: made once."""
    key = (grouped, tail_newline)
    if key not in _shared:
        w = _named(make_workload(CONFIGS["config1"], seed=31, shuffled=not grouped, n_records=3_000))
        text = sam_text(tmp_path, w, tail_newline=tail_newline)
        skip = D.header_len(text)
        s, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        _shared[key] = (w, text, skip, run_workload(w, use_qnames=True), want)
    return _shared[key]


def test_the_inputs_hold_what_they_are_named_for(tmp_path):
    """Default gzip of this text is one final dynamic block; memLevel 1 gives about a hundred; Z_FIXED fixed blocks only; a
    sync flush an empty stored block behind each dynamic one; level 0 stored blocks only."""
    _, text, _, _, _ = case(tmp_path, True)
    types = {k: D.count_types(D.member_blocks(D.copy_of(text, k))) for k in ("default", "mem1", "fixed", "sync", "stored")}
    assert types["default"] == {0: 0, 1: 0, 2: 1}
    assert types["mem1"][2] >= 50 and types["mem1"][0] == types["mem1"][1] == 0
    assert types["fixed"][1] >= 50 and types["fixed"][2] == 0
    assert types["sync"][0] >= 20 and types["sync"][2] >= 20
    assert types["stored"][0] >= 7 and types["stored"][1] == types["stored"][2] == 0


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cut,force", [("one", "gzip_chunk=2048"), ("random", "gzip_chunk=2048,gzip_round=1"), ("60k", "gzip_chunk=4096")])
def test_gzip_sam_bytes_give_the_partials_of_the_text(tmp_path, monkeypatch, grouped, kind, cut, force):
    """The file's bytes pushed whole, cut at random offsets (inside headers, blocks and trailers; with gzip_round=1 every
    push is decoded as far as it goes and the rest waits for the next push), or in 60 kB windows; one member of each kind of
    block, or members of different kinds back to back with an empty one among them."""
    w, text, skip, o, want = case(tmp_path, grouped)
    blob = D.copy_of(text, kind)
    cuts = {"one": [], "random": random_cuts(len(blob), 7, 1, 9_000), "60k": list(range(60_000, len(blob), 60_000))}[cut]
    forced(monkeypatch, force)
    s, got = profile_of(w, grouped, lambda s: s.push_gzip_sam_bytes(blob, skip=skip, cuts=cuts))
    st = s.gzip_stats()
    assert got == want
    assert_matches_oracle(s, o)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob)
    assert st["members"] == (4 if kind == "members" else 1)
    if kind == "default":
        assert (st["chunks"], st["dynamic_blocks"]) == (1, 1) or cut == "random"   # (the one-chunk case)
    if kind == "mem1" and cut == "one":
        assert st["chunks"] >= 8 and st["dropped"] == 0 and st["resolved_bytes"] > 0, st
    if kind == "fixed":
        assert st["fixed_blocks"] >= 50 and st["dynamic_blocks"] == 0 and st["candidates"] == 0, st
    if kind == "stored":
        assert st["stored_blocks"] >= 7 and st["candidates"] == 0, st
    if kind == "sync":
        assert st["stored_blocks"] >= 20 and st["dynamic_blocks"] >= 20, st
    if cut == "random":
        assert st["rounds"] > st["members"], st
    s.close()


@pytest.mark.parametrize("force", ["gzip_chunk=2048", "gzip_chunk=2048,gzip_round=1"])
def test_last_line_without_newline(tmp_path, monkeypatch, force):
    """The text's last line has no newline: it is a line all the same -- also when the last push carries no byte."""
    w, text, skip, o, _ = case(tmp_path, True, tail_newline=False)
    forced(monkeypatch, force)
    for empty_last in (False, True):
        for kind in ("mem1", "members"):
            s, _ = profile_of(w, True, lambda s: s.push_gzip_sam_bytes(D.copy_of(text, kind), skip=skip, window=5_000, empty_last=empty_last))
            assert_matches_oracle(s, o)
            s.close()


def test_forced_false_starts_change_nothing(tmp_path, monkeypatch):
    """SLIMM_FORCE gzip_false_starts: chunk starts a few bits into every real block and every 997 bits are walked and dropped
    by the chain; every output is that of the run without them."""
    w, text, skip, _, want = case(tmp_path, True)
    blob = D.copy_of(text, "members")
    forced(monkeypatch, "gzip_chunk=2048,gzip_false_starts=997")
    s, got = profile_of(w, True, lambda s: s.push_gzip_sam_bytes(blob, skip=skip, window=7_000))
    st = s.gzip_stats()
    assert got == want
    assert st["forced_starts"] > 0 and st["dropped"] > 0, st
    s.close()


def test_a_block_header_inside_a_member_header_starts_no_chunk(tmp_path, monkeypatch):
    """A second member whose FEXTRA field holds the first 200 bytes of a real dynamic block: a candidate found there is
    dropped (or none is found), and the outputs are those of the text."""
    w, text, skip, _, want = case(tmp_path, True)
    half = len(text) // 2
    first = D.member(text[:half], memLevel=1)
    bl = [b for b in D.member_blocks(first) if b[1] == 2 and not b[2]]
    at = 10 + bl[3][0] // 8
    blob = first + D.member(text[half:], memLevel=1, extra=first[at:at + 200])
    real = len(bl) + sum(1 for b in D.member_blocks(D.member(text[half:], memLevel=1)) if b[1] == 2 and not b[2])
    forced(monkeypatch, "gzip_chunk=2048")
    s, got = profile_of(w, True, lambda s: s.push_gzip_sam_bytes(blob, skip=skip))
    st = s.gzip_stats()
    assert got == want
    assert st["dropped"] >= 1 or st["candidates"] == real, (st, real)
    assert st["members"] == 2
    s.close()


def both_ways(w, blob, text, skip=0, **kw):
    """The profile of a crafted member's text through the gzip push and through the text push: equal, and the gzip stats."""
    assert zlib.decompress(blob, 31) == text
    s1, want = profile_of_any(w, lambda s: s.push_sam_bytes(text[skip:]))
    s2, got = profile_of_any(w, lambda s: s.push_gzip_sam_bytes(blob, skip=skip, **kw))
    st = s2.gzip_stats()
    assert got == want
    s1.close()
    s2.close()
    return st


def profile_of_any(w, push):
    s = Slimm.for_workload(w, device=0, grouped=False)
    s.set_reference_names(w.ref_names)
    n = push(s)
    s.get_profiles()
    return s, (n, integers(s))


def test_crafted_copies_reach_in_front_of_their_chunk(tmp_path, monkeypatch):
    """A chunk that starts with a tiny dynamic block and then copies 258 bytes at distance 32 768 (the farthest byte of the
    chunk in front), and a run at distance 1 longer than the distance; a copy whose source straddles the chunk's start."""
    w, text, skip, _, _ = case(tmp_path, False)
    body = text[skip:]
    blob, crafted, before = D.far_copy_member(body, w.ref_names[0].encode())
    forced(monkeypatch, f"gzip_chunk={before}")
    st = both_ways(w, blob, crafted)
    assert st["chunks"] == 2 and st["dropped"] == 0 and st["resolved_bytes"] == 512 and st["fixed_blocks"] == 2, st
    blob, crafted, before = D.straddling_copy_member(body)
    forced(monkeypatch, f"gzip_chunk={before}")
    st = both_ways(w, blob, crafted)
    assert st["chunks"] == 2 and st["dropped"] == 0 and st["resolved_bytes"] == 20, st


def test_copies_of_copies_across_three_chunks(tmp_path, monkeypatch):
    """20 kB of lines thirty times at memLevel 1: chunk k copies what chunk k - 1 copied from chunk k - 2."""
    w, text, skip, _, _ = case(tmp_path, False)
    body = text[skip:]
    block = body[:body.index(b"\n", 20_000) + 1]
    crafted = block * 30
    blob = D.member(crafted, memLevel=1)
    forced(monkeypatch, "gzip_chunk=512")
    st = both_ways(w, blob, crafted, cuts=random_cuts(len(blob), 3, 100, 3_000))
    assert st["chunks"] >= 3 and st["resolved_bytes"] > len(block), st


def push_error(w, blob, skip, **kw):
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception) as e:
        s.push_gzip_sam_bytes(blob, skip=skip, **kw)
    s.close()
    return str(e.value)


def test_damage_is_an_error_and_gzip_does_not_mix_with_bam(tmp_path, monkeypatch):
    w, text, skip, _, _ = case(tmp_path, True)
    forced(monkeypatch, "gzip_chunk=2048")
    blob = D.copy_of(text, "mem1")
    stored = bytearray(D.copy_of(text, "stored"))
    stored[10 + 3] ^= 0x01   # (NLEN of the first stored block)
    huff = bytearray(blob)
    huff[len(blob) // 2] ^= 0x10
    cases = {
        "huffman_bit": (bytes(huff), CORRUPT),
        "stored_nlen": (bytes(stored), CORRUPT + "invalid stored block lengths"),
        "crc": (D.member(text, memLevel=1, crc=zlib.crc32(text) ^ 1), CORRUPT + "incorrect data check"),
        "isize": (D.member(text, memLevel=1, isize=len(text) + 1), CORRUPT + "incorrect length check"),
        "two_thirds": (blob[:2 * len(blob) // 3], TRUNCATED),
        "inside_trailer": (blob[:-3], TRUNCATED),
        "junk": (blob + b"\x00junk", CORRUPT),
        "too_far_back": (D.too_far_back_member(), CORRUPT + "invalid distance too far back"),
        "too_far_back_in_member_2": (D.member(text[:skip + 5_000]) + D.too_far_back_member(), CORRUPT + "invalid distance too far back"),
    }
    for name, (data, word) in cases.items():
        for kw in (dict(), dict(window=3_000)):
            msg = push_error(w, data, skip, **kw)
            assert word in msg, (name, kw, msg)
    # gzip bytes behind BAM bytes of the same file, and text behind gzip bytes
    got = C.c_uint64()
    filler = np.zeros(64, dtype=np.uint8)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_bam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 0, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_gzip_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_gzip_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_sam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 10, 1, C.byref(got)) == SLIMM_E_INVALID
    s.close()
