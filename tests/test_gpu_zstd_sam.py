"""zstd-compressed SAM on a real MI355X: slimm_push_zstd_sam_bytes (the file's bytes, cut anywhere; frames and blocks walked
on the host, literals and sequences decoded a wave per block, the text built in parallel over its bytes and resolved by
pointer doubling, the text found and decoded as SAM) against slimm_push_sam_bytes on the same text and the CPU oracle.
slimm_get_zstd_stats says that an input reached what it was built for.  The inputs: tests/sam_zst.py -- the committed
compressor-made files of tests/golden/zstd and frames written in Python; libzstd is not needed."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from tests import sam_zst as Z
from tests.helpers import assert_matches_oracle
from tests.test_gpu_compressed_sam import integers, profile_of

pytestmark = pytest.mark.gpu

SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)
WORDS = "zstd-compressed input is not supported unless it decodes: "
GOLDEN = ["l3", "l19", "wlog10"]
WRITTEN = ["raw_blocks", "rle_blocks", "plain_header", "single_segment", "frames", "skippable_first"]


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


def case(tmp_path, grouped, n_records=3_000, tail_newline=True):
    """The text (3 000 records, or the 400 of the windowLog-10 file), its header's length, the oracle's run and the profile
    of the plain text: made once."""
    key = (grouped, n_records, tail_newline)
    if key not in _shared:
        w = Z.case_workload(grouped, n_records)
        text = Z.case_text(tmp_path, grouped, n_records)
        text = text if tail_newline else text[:-1]
        skip = Z.header_len(text)
        s, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        _shared[key] = (w, text, skip, run_workload(w, use_qnames=True), want)
    return _shared[key]


def blob_of(tmp_path, grouped, kind):
    """(the case, the zstd bytes) of an input kind."""
    tag = "grouped" if grouped else "any"
    if kind in GOLDEN:
        c = case(tmp_path, grouped, 400 if kind == "wlog10" else 3_000)
        name = f"short_{tag}_wlog10.sam.zst" if kind == "wlog10" else f"config1_{tag}_{kind}.sam.zst"
        return c, Z.golden(name)
    c = case(tmp_path, grouped)
    return c, Z.written_copies(c[1])[kind]


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind", GOLDEN + WRITTEN)
@pytest.mark.parametrize("cut,force", [("one", ""), ("random", "zstd_round=1"), ("60k", "")])
def test_zstd_sam_bytes_give_the_partials_of_the_text(tmp_path, monkeypatch, grouped, kind, cut, force):
    """The file's bytes pushed whole, cut at random offsets (inside frame headers, block headers, blocks and checksums; with
    zstd_round=1 every push is decoded as far as it goes and the rest waits for the next push), or in 60 kB windows."""
    (w, text, skip, o, want), blob = blob_of(tmp_path, grouped, kind)
    cuts = {"one": [], "random": random_cuts(len(blob), 7, 1, 9_000), "60k": list(range(60_000, len(blob), 60_000))}[cut]
    forced(monkeypatch, force)
    s, got = profile_of(w, grouped, lambda s: s.push_zstd_sam_bytes(blob, skip=skip, cuts=cuts))
    st = s.zstd_stats()
    assert got == want
    assert_matches_oracle(s, o)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob)
    census = Z.census(blob)
    assert st["frames"] == census["frames"] and st["skippable"] == census["skippable"]
    assert (st["raw_blocks"], st["rle_blocks"], st["compressed_blocks"]) == (census["raw"], census["rle"], census["compressed"])
    assert st["checksums"] == sum(1 for f in Z.walk(blob) if f.get("checksum_at") is not None)
    if kind == "l3":
        assert st["treeless"] > 0 and st["huffman_trees"] > 0 and st["fse_tables"] > 0 and st["sequences"] > 1_000 and st["front_bytes"] > 0, st
    if kind == "l19":
        assert st["repeated"] > 0, st
    if kind == "wlog10":
        assert st["predefined"] > 100 and st["treeless"] > 40 and st["plain_literals"] > 0 and st["compressed_blocks"] >= 50, st
    if kind == "raw_blocks":
        assert st["raw_blocks"] >= 7 and st["compressed_blocks"] == 0, st
    if kind == "rle_blocks":
        assert st["rle_blocks"] > 0, st
    if kind == "frames":
        assert st["frames"] == 4 and st["skippable"] == 1, st
    if kind == "skippable_first":
        assert st["skippable"] == 1, st
    if cut == "random" and len(blob) > 20_000:
        assert st["rounds"] > 1, st
    s.close()


@pytest.mark.parametrize("kind", ["l3", "wlog10"])
def test_copies_reach_into_the_history_of_an_earlier_round(tmp_path, monkeypatch, kind):
    """SLIMM_FORCE zstd_round_text=N: rounds of a few blocks of text; what a block copies from blocks of an earlier round
    comes from the history kept on the device (the frame's last window of text)."""
    (w, text, skip, o, want), blob = blob_of(tmp_path, True, kind)
    forced(monkeypatch, "zstd_round_text=4096" if kind == "wlog10" else "zstd_round_text=131072")
    s, got = profile_of(w, True, lambda s: s.push_zstd_sam_bytes(blob, skip=skip))
    st = s.zstd_stats()
    assert got == want
    assert_matches_oracle(s, o)
    assert st["rounds"] >= 3 and st["history_bytes"] > 0 and st["front_bytes"] >= st["history_bytes"], st
    s.close()


@pytest.mark.parametrize("force", ["", "zstd_round=1"])
def test_last_line_without_newline(tmp_path, monkeypatch, force):
    """The text's last line has no newline: it is a line all the same -- also when the last push carries no byte."""
    w, text, skip, o, _ = case(tmp_path, True, tail_newline=False)
    forced(monkeypatch, force)
    blob = Z.raw_frame(text, step=40_000, rle=True)
    for empty_last in (False, True):
        s, _ = profile_of(w, True, lambda s: s.push_zstd_sam_bytes(blob, skip=skip, window=5_000, empty_last=empty_last))
        assert_matches_oracle(s, o)
        s.close()


def profile_of_any(w, push):
    s = Slimm.for_workload(w, device=0, grouped=False)
    s.set_reference_names(w.ref_names)
    n = push(s)
    s.get_profiles()
    return s, (n, integers(s))


def test_a_run_of_100_000_bytes_at_offset_1_resolves_within_the_bound(tmp_path, monkeypatch):
    """One match of 100 000 bytes at offset 1 -- the chain of copies is as long as the run --, in a SEQ field: pointer doubling
    resolves it in at most ceil(log2(text + history)) + 1 passes (fewer where a pass reads what it has just shortened)."""
    w, text, skip, _, _ = case(tmp_path, False)
    body = text[skip:]
    lines = body.split(b"\n")
    f = lines[0].split(b"\t")
    f[5], f[9], f[10] = b"100001M", b"A", b"*"
    front = b"\n".join(lines[1:40]) + b"\n" + b"\t".join(f[:10])
    back = b"\t" + b"\t".join(f[10:]) + b"\n" + b"\n".join(lines[40:80]) + b"\n"
    blob, crafted = Z.run_frame(front, 100_000, back)
    assert crafted.count(b"A" * 100_001) == 1
    forced(monkeypatch, "")
    s1, want = profile_of_any(w, lambda s: s.push_sam_bytes(crafted))
    for cuts in ([], random_cuts(len(blob), 5, 1, 3_000)):
        s2, got = profile_of_any(w, lambda s: s.push_zstd_sam_bytes(blob, cuts=cuts))
        st = s2.zstd_stats()
        assert got == want
        bound = (len(crafted) - 1).bit_length() + 1
        assert 1 <= st["passes"] <= bound, (st, bound)
        # (of the run only its first byte copies from in front of its block: every other one from the byte before it)
        assert st["rle_tables"] == 3 and st["front_bytes"] == 1 and st["checksums"] == 1, st
        s2.close()
    s1.close()


def push_error(w, blob, skip, **kw):
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception) as e:
        s.push_zstd_sam_bytes(blob, skip=skip, **kw)
    s.close()
    return str(e.value)


def flipped(blob, at, bit=0x10):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def test_damage_is_an_error_in_the_host_readers_words_and_the_context_stays_usable(tmp_path, monkeypatch):
    (w, text, skip, o, want), blob = blob_of(tmp_path, True, "l3")
    forced(monkeypatch, "")
    fr = Z.walk(blob)[0]
    first = next(b for b in fr["blocks"] if b["type"] == 2 and b.get("huf_at") and b.get("fse_at"))
    raw = Z.raw_frame(text)
    run, _ = Z.run_frame(text[:skip + 500], 70_000, b"\n")
    far = run.replace(Z.one_match_block(70_000, 1), Z.one_match_block(70_000, len(text)))   # (an offset in front of the frame's start)
    cases = {
        "two_thirds": (blob[:2 * len(blob) // 3], "truncated"),
        "inside_frame_header": (blob[:5], "truncated"),
        "inside_block_header": (blob[:first["at"] + 2], "truncated"),
        "inside_checksum": (blob[:-2], "truncated"),
        "huffman_description": (flipped(blob, first["huf_at"], 0x80), ""),
        "fse_description": (flipped(blob, first["fse_at"], 0x0f), ""),
        "sequence_stream": (flipped(blob, first["bits_at"] + 20), ""),
        "padding": (flipped(blob, first["at"] + 3 + first["size"] - 1, blob[first["at"] + 3 + first["size"] - 1]), "padding bit"),
        "checksum": (flipped(blob, fr["checksum_at"]), "content checksum mismatch"),
        "content_size": (Z.raw_frame(text, wrong_size=True), "content size mismatch"),
        "dictionary": (Z.frame_header(None, False, 17, dict_id=5) + Z.block(0, text, last=True)[:100], "a dictionary"),
        "window_256m": (Z.frame_header(None, False, 28) + Z.block(0, b"x", last=True), "128 MiB"),
        "reserved_bit": (flipped(raw, 4, 0x08), "reserved bit"),
        "reserved_block": (flipped(raw, Z.walk(raw)[0]["blocks"][0]["at"], 0x06), "reserved block type"),
        "block_too_large": (Z.frame_header(None, False, 10) + Z.block(0, text[:2_000], last=True), "larger than its maximum"),
        "offset_too_far": (far, "offset beyond"),
        "junk": (blob + b"junk!", "start no frame"),
    }
    for name, (data, word) in cases.items():
        for kw in (dict(), dict(window=3_000)):
            msg = push_error(w, data, skip, **kw)
            assert WORDS in msg and word in msg, (name, kw, msg)
    # a failed file, a reset, a good file: the context is as good as new
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception):
        s.push_zstd_sam_bytes(cases["sequence_stream"][0], skip=skip)
    s.reset()
    assert s.push_zstd_sam_bytes(blob, skip=skip) == len(w.records)
    s.get_profiles()
    assert integers(s) == want
    assert_matches_oracle(s, o)
    s.close()


def test_zstd_does_not_mix_with_other_forms_and_is_not_cut_by_byte_range(tmp_path, monkeypatch):
    (w, text, skip, _, _), blob = blob_of(tmp_path, True, "l3")
    forced(monkeypatch, "")
    got = C.c_uint64()
    filler = np.zeros(64, dtype=np.uint8)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_bam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 0, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_zstd_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_zstd_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_sam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 10, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "do not mix" in s.L.slimm_last_error(s.ctx).decode()
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_set_input_mid_file(s.ctx, 0, 1) == SLIMM_OK
    assert s.L.slimm_push_zstd_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "a zstd stream is not cut by byte range" in s.L.slimm_last_error(s.ctx).decode()
    s.close()


@pytest.mark.parametrize("force", ["zstd_round=1", ""])
def test_a_stream_that_waited_across_rounds_and_ends_short_is_truncated(tmp_path, monkeypatch, force):
    """The file cut inside a frame header, a block header, a block, the checksum, between two frames' bytes: pushed in pieces
    that are decoded as far as they go (zstd_round=1: the rest waits), then closed -- by the last piece or by an empty last
    push -- it is `truncated`, never a file with fewer records."""
    (w, text, skip, _, _), blob = blob_of(tmp_path, True, "l3")
    forced(monkeypatch, force)
    fr = Z.walk(blob)[0]
    blocks = fr["blocks"]
    two = blob + blob
    cases = {
        "frame_header": blob[:5],
        "block_header": blob[:blocks[1]["at"] + 2],
        "block": blob[:blocks[2]["at"] + 3 + blocks[2]["size"] // 2],
        "two_thirds": blob[:2 * len(blob) // 3],
        "checksum": blob[:-2],
        "no_checksum": blob[:-4],
        "second_frame_magic": two[:len(blob) + 2],
        "second_frame_block": two[:len(blob) + blocks[1]["at"] + 1],
    }
    for name, data in cases.items():
        for cuts in ([len(data) // 2], [len(data) // 3, len(data) - 1], random_cuts(len(data), 9, 1, 9_000)):
            for empty_last in (True, False):
                msg = push_error(w, data, skip, cuts=cuts, empty_last=empty_last)
                assert WORDS in msg and "truncated" in msg, (name, cuts[:3], empty_last, msg)


@pytest.mark.parametrize("kind,step,force", [("raw", 50_000, "zstd_round_text=131072"), ("raw", 10_000, "zstd_round_text=20000"),
                                             ("rle", 30_000, "zstd_round_text=65536"), ("raw", 50_000, "zstd_round_text=131072,zstd_round=1")])
def test_rounds_that_read_equally_many_bytes_go_on_to_the_files_end(tmp_path, monkeypatch, kind, step, force):
    """Raw blocks of one size under a small zstd_round_text: round after round reads the same number of compressed bytes
    and ends inside the frame; every one of them is decoded, pushed whole or in pieces."""
    w, text, skip, o, want = case(tmp_path, True)
    blob = Z.raw_frame(text, step=step, rle=kind == "rle")
    for cuts in ([], random_cuts(len(blob), 13, 1, 150_000)):
        forced(monkeypatch, force)
        s, got = profile_of(w, True, lambda s: s.push_zstd_sam_bytes(blob, skip=skip, cuts=cuts))
        st = s.zstd_stats()
        assert got == want
        assert_matches_oracle(s, o)
        assert st["text_bytes"] == len(text) and st["rounds"] >= 4, st
        s.close()
