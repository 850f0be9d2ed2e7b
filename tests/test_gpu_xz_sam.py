"""xz-compressed SAM on a real MI355X: slimm_push_xz_sam_bytes (the file's bytes, cut anywhere; streams, blocks and LZMA2
chunk headers walked on the host, every block decoded by a lane of its own into the round's text, its CRC32 or CRC64 folded
from pieces, every index compared with its blocks, the text found and decoded as SAM) against slimm_push_sam_bytes on the
same text and the CPU oracle.  slimm_get_xz_stats must equal the census of the tests' own walker, and says that an input
reached what it was built for.  The inputs: tests/sam_xz.py -- the committed compressor-made files of tests/golden/xz and
containers written in Python; neither an `xz` binary nor liblzma is needed."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from tests import sam_xz as X
from tests.helpers import assert_matches_oracle
from tests.test_gpu_compressed_sam import integers, profile_of

pytestmark = pytest.mark.gpu

SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)
WORDS = "xz-compressed input is not supported unless it decodes: "
GOLDEN = sorted(X.GOLDEN_KINDS)
WRITTEN = ["stored_chunks", "reblocked", "two_streams_padded", "empty_stream"]
CENSUS = {"streams": "streams", "blocks": "blocks", "lzma_chunks": "lzma_chunks", "raw_chunks": "raw_chunks", "check_none": "check_none",
          "check_crc32": "check_crc32", "check_crc64": "check_crc64", "sha256_unverified": "sha256_unverified", "text_bytes": "text",
          "compressed_bytes": "compressed", "state_resets": "state_resets", "prop_changes": "prop_changes", "odd_props": "odd_props",
          "index_records": "index_records"}


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


def case(tmp_path, grouped, n_records=1_000, tail_newline=True):
    """The text, its header's length, the oracle's run and the profile of the plain text: made once per text."""
    key = (grouped, n_records, tail_newline)
    if key not in _shared:
        w = X.case_workload(grouped, n_records)
        text = X.case_text(tmp_path, grouped, n_records)
        text = text if tail_newline else text[:-1]
        skip = X.header_len(text)
        s, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        _shared[key] = (w, text, skip, run_workload(w, use_qnames=True), want)
    return _shared[key]


def blob_of(tmp_path, grouped, kind):
    """(the case, the xz bytes) of an input kind."""
    tag = "grouped" if grouped else "any"
    if kind in X.GOLDEN_KINDS:
        n, name = X.GOLDEN_KINDS[kind]
        return case(tmp_path, grouped, n), X.golden(name.format(tag))
    c = case(tmp_path, grouped)
    return c, X.written_copies(c[1], tag)[kind]


def assert_census(st, blob):
    want = X.census(blob)
    assert {k: st[k] for k in CENSUS} == {k: want[v] for k, v in CENSUS.items()}, (st, want)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind", GOLDEN + WRITTEN)
@pytest.mark.parametrize("cut,force", [("one", ""), ("random", "xz_round=1"), ("60k", "")])
def test_xz_sam_bytes_give_the_partials_of_the_text(tmp_path, monkeypatch, grouped, kind, cut, force):
    """The file's bytes pushed whole, cut at random offsets (inside stream, block and chunk headers, chunks, checks, indexes
    and footers; with xz_round=1 every push is decoded as far as it goes and the rest waits for the next push), or in 60 kB
    windows."""
    (w, text, skip, o, want), blob = blob_of(tmp_path, grouped, kind)
    cuts = {"one": [], "random": random_cuts(len(blob), 7, 1, 9_000), "60k": list(range(60_000, len(blob), 60_000))}[cut]
    forced(monkeypatch, force)
    s, got = profile_of(w, grouped, lambda s: s.push_xz_sam_bytes(blob, skip=skip, cuts=cuts))
    st = s.xz_stats()
    assert got == want
    assert_matches_oracle(s, o)
    assert_census(st, blob)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob)
    assert st["max_dist"] <= len(text) and (st["match_bytes"] > 0) == (st["lzma_chunks"] > 0), st
    if kind == "mt":
        assert st["blocks"] >= 8, st
    if kind == "one":
        assert st["lzma_chunks"] >= 2 and st["lzma_chunks"] > st["state_resets"], st   # (a chunk that resets nothing)
    if kind in ("lc0lp2", "lc4"):
        assert st["odd_props"] >= 1, st
    if kind == "stored_chunks":
        assert st["raw_chunks"] > 1 and st["lzma_chunks"] == 0, st
    if kind == "two_streams_padded":
        assert st["streams"] == 2, st
    if kind == "sha256":
        assert st["sha256_unverified"] == st["blocks"] > 0, st
    if cut == "random" and len(blob) > 20_000:   # (a block waits until all its bytes have come: a file of one block is one round)
        assert st["rounds"] > 1 if st["blocks"] > 1 else st["rounds"] == 1, st
    s.close()


@pytest.mark.parametrize("force,rounds", [("xz_round_text=40000", 14), ("xz_round_text=1,xz_round=1", 14), ("xz_round_text=100000", 4)])
def test_a_round_takes_the_blocks_that_fit_and_the_next_round_the_rest(tmp_path, monkeypatch, force, rounds):
    """SLIMM_FORCE xz_round_text=N: a round ends in front of the block that would take its text past N -- one block alone
    when it is larger --, and the next round starts there."""
    (w, text, skip, o, want), blob = blob_of(tmp_path, True, "mt")
    forced(monkeypatch, force)
    for cuts in ([], random_cuts(len(blob), 3, 1, 5_000)):
        s, got = profile_of(w, True, lambda s: s.push_xz_sam_bytes(blob, skip=skip, cuts=cuts))
        st = s.xz_stats()
        assert got == want
        assert_matches_oracle(s, o)
        assert_census(st, blob)
        assert st["rounds"] >= rounds, st
        s.close()


@pytest.mark.parametrize("force", ["", "xz_round=1"])
def test_last_line_without_newline(tmp_path, monkeypatch, force):
    """The text's last line has no newline: it is a line all the same, in a window of its own -- also when the last push
    carries no byte."""
    w, text, skip, o, _ = case(tmp_path, True, tail_newline=False)
    forced(monkeypatch, force)
    blob = X.stored_chunks(text, step=30_000, check=1)
    for empty_last in (False, True):
        s, _ = profile_of(w, True, lambda s: s.push_xz_sam_bytes(blob, skip=skip, window=5_000, empty_last=empty_last))
        assert_matches_oracle(s, o)
        s.close()


def flipped(blob, at, bit=0x10):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def with_byte(blob, at, v):
    b = bytearray(blob)
    b[at] = v
    return bytes(b)


def damaged(text, tag):
    """{name: (bytes, the cause's words)}: the reblocked container (three compressor-made blocks, CRC32) cut behind every
    structural element and damaged in every kind of place, and what the decoder does not take."""
    blob = X.written_copies(text, tag)["reblocked"]
    s = X.walk(blob)[0]
    b0, b1 = s["blocks"][0], s["blocks"][1]
    ch = b0["chunks"][0]
    no_reset = X.stream_of([(X.block_header(), X.raw_chunks(text, 40_000, first_control=2), text)])
    return blob, {
        "inside_the_stream_header": (blob[:7], "stream header at byte 0: truncated"),
        "behind_the_stream_header": (blob[:12], "block header at byte 12: truncated"),
        "inside_a_block_header": (blob[:b0["at"] + 3], "block header at byte 12: truncated"),
        "behind_a_block_header": (blob[:b0["data_at"]], "block at byte 12: truncated"),
        "inside_a_chunk_header": (blob[:ch["at"] + 2], "block at byte 12: truncated"),
        "inside_a_chunk": (blob[:ch["at"] + 100], "block at byte 12: truncated"),
        "behind_the_end_marker": (blob[:b0["pad_at"]], "block at byte 12: truncated"),
        "inside_the_check": (blob[:b0["check_at"] + 2], "block at byte 12: truncated"),
        "between_blocks": (blob[:b1["at"]], "truncated"),
        "inside_the_index": (blob[:s["index_at"] + 3], "index at byte"),
        "behind_the_index": (blob[:s["footer_at"]], "stream footer at byte"),
        "inside_the_footer": (blob[:-3], "stream footer at byte"),
        "stream_header": (flipped(blob, 7, 0x01), "header CRC32 mismatch"),
        "block_header": (flipped(blob, b0["at"] + 2), "block header CRC32 mismatch"),
        "index": (flipped(blob, s["index_at"] + 2), "index CRC32 mismatch"),
        "footer": (flipped(blob, s["footer_at"] + 5), "footer CRC32 mismatch"),
        "check": (flipped(blob, b0["check_at"]), "block at byte 12: check mismatch"),
        "lzma_data": (flipped(blob, ch["at"] + ch["header"] + 40), "block at byte 12: "),
        "one_more_byte_of_text": (with_byte(blob, ch["at"] + 2, (blob[ch["at"] + 2] + 1) & 0xff), "block at byte 12: "),
        "no_dictionary_reset": (with_byte(blob, ch["at"], 0xC0 | (blob[ch["at"]] & 0x1f)), "a block's first chunk does not reset the dictionary"),
        "no_dictionary_reset_stored": (no_reset, "a block's first chunk does not reset the dictionary"),
        "lc_plus_lp_5": (with_byte(blob, ch["at"] + 5, 4 + 9 * (1 + 5 * 2)), "bad LZMA properties (lc + lp > 4)"),
        "bcj": (X.golden(X.REFUSED_KIND[1].format(tag)), "a filter chain other than LZMA2 alone (filter id 4)"),
        "garbage_behind": (blob + b"garbage!", "bytes behind the last stream that are neither padding nor a stream"),
        "index_of_other_blocks": (blob[:s["index_at"]] + X.index_of([(a + 4, u) for a, u in s["records"]]) + blob[s["footer_at"]:],
                                  "index does not match the blocks"),
    }


NAMES = ["inside_the_stream_header", "behind_the_stream_header", "inside_a_block_header", "behind_a_block_header", "inside_a_chunk_header",
         "inside_a_chunk", "behind_the_end_marker", "inside_the_check", "between_blocks", "inside_the_index", "behind_the_index", "inside_the_footer",
         "stream_header", "block_header", "index", "footer", "check", "lzma_data", "one_more_byte_of_text", "no_dictionary_reset",
         "no_dictionary_reset_stored", "lc_plus_lp_5", "bcj", "garbage_behind", "index_of_other_blocks"]


def test_every_kind_of_damage_has_a_case():
    assert sorted(damaged_names()) == sorted(NAMES)


def damaged_names():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        return list(damaged(X.case_text(d, True, 1_000), "grouped")[1])


@pytest.mark.parametrize("name", NAMES)
def test_damage_is_an_error_in_the_host_readers_words_and_the_context_stays_usable(tmp_path, monkeypatch, name):
    """SLIMM_E_INVALID with the words and the named cause, pushed whole and in 3 000-byte pieces; then slimm_reset and a good
    file on the same context give the right profile."""
    w, text, skip, o, want = case(tmp_path, True)
    forced(monkeypatch, "")
    good, cases = damaged(text, "grouped")
    data, word = cases[name]
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    for kw in (dict(), dict(window=3_000)):
        with pytest.raises(Exception) as e:
            s.push_xz_sam_bytes(data, skip=skip, **kw)
        assert WORDS in str(e.value) and word in str(e.value), (name, kw, str(e.value))
        s.reset()
    assert s.push_xz_sam_bytes(good, skip=skip) == len(w.records)
    s.get_profiles()
    assert integers(s) == want
    assert_matches_oracle(s, o)
    assert_census(s.xz_stats(), good)
    s.close()


def test_xz_does_not_mix_with_other_forms_and_is_not_cut_by_byte_range(tmp_path, monkeypatch):
    (w, text, skip, _, _), blob = blob_of(tmp_path, True, "l0")
    forced(monkeypatch, "")
    got = C.c_uint64()
    filler = np.zeros(64, dtype=np.uint8)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_xz_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_sam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 10, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "do not mix" in s.L.slimm_last_error(s.ctx).decode()
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_set_input_mid_file(s.ctx, 0, 1) == SLIMM_OK
    assert s.L.slimm_push_xz_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "an xz stream is not cut by byte range" in s.L.slimm_last_error(s.ctx).decode()
    s.close()


@pytest.mark.parametrize("force", ["xz_round=1", ""])
def test_a_stream_that_waited_across_rounds_and_ends_short_is_truncated(tmp_path, monkeypatch, force):
    """The file cut inside a header, a chunk, a check, the index, the footer: pushed in pieces that are decoded as far as they
    go, then closed -- by the last piece or by an empty last push -- it is `truncated`, never a file with fewer records."""
    w, text, skip, _, _ = case(tmp_path, True)
    forced(monkeypatch, force)
    _, cases = damaged(text, "grouped")
    for name in NAMES[:12]:
        data = cases[name][0]
        for cuts in ([len(data) // 2], random_cuts(len(data), 9, 1, 4_000)):
            for empty_last in (True, False):
                s = Slimm.for_workload(w, device=0, grouped=True)
                s.set_reference_names(w.ref_names)
                with pytest.raises(Exception) as e:
                    s.push_xz_sam_bytes(data, skip=skip, cuts=cuts, empty_last=empty_last)
                s.close()
                assert WORDS in str(e.value) and "truncated" in str(e.value), (name, cuts[:3], empty_last, str(e.value))
