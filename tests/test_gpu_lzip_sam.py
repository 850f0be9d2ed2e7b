"""lzip-compressed SAM on a real MI355X: slimm_push_lzip_sam_bytes (the file's bytes, cut anywhere; the members found on the
host by their trailers' member_size, every member decoded by a lane of its own into the round's text, its CRC32 folded from
pieces and held against its trailer, the text found and decoded as SAM) against slimm_push_sam_bytes on the same text and the
CPU oracle.  slimm_get_lzip_stats must equal the census of the tests' own walker.  The inputs: tests/sam_lzip.py -- the
committed files of tests/golden/lzip and members written with Python's `lzma` -- and tests/lzip_directed.py; no `lzip`
binary is needed.  SLIMM_FORCE keys named here: lzip_round, lzip_round_text."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from tests import lzip_directed as LD
from tests import sam_lzip as Z
from tests.helpers import assert_matches_oracle
from tests.test_gpu_compressed_sam import integers, profile_of

pytestmark = pytest.mark.gpu

SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)
WORDS = "lzip-compressed input is not supported unless it decodes: "
# (kind, grouped): the committed files in the orders they exist in, the written ones in both
KINDS = [(k, tag == "grouped") for k, (_, _, tags) in sorted(Z.GOLDEN_KINDS.items()) for tag in tags] + \
        [(k, g) for k in ("three_members", "empty_first_and_last", "every_fraction") for g in (True, False)]
CENSUS = ("members", "empty_members", "crc32_checked", "max_dict", "text_bytes", "compressed_bytes")


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
        w = Z.case_workload(grouped, n_records)
        text = Z.case_text(tmp_path, grouped, n_records)
        text = text if tail_newline else text[:-1]
        skip = Z.header_len(text)
        s, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        _shared[key] = (w, text, skip, run_workload(w, use_qnames=True), want)
    return _shared[key]


def blob_of(tmp_path, grouped, kind):
    """(the case, the lzip bytes) of an input kind."""
    if kind in Z.GOLDEN_KINDS:
        n, name, _ = Z.GOLDEN_KINDS[kind]
        return case(tmp_path, grouped, n), Z.golden(name.format("grouped" if grouped else "any"))
    c = case(tmp_path, grouped)
    return c, Z.written_copies(c[1])[kind]


def assert_census(st, blob):
    want = Z.census(blob)
    assert {k: st[k] for k in CENSUS} == want, (st, want)


def directed(tmp_path):
    """The 50-record case and its directed inputs."""
    if "directed" not in _shared:
        c = case(tmp_path, True, 50)
        _shared["directed"] = (c, LD.INPUTS(c[1][:c[2]], c[1][c[2]:]))
    return _shared["directed"]


@pytest.mark.parametrize("kind,grouped", KINDS)
@pytest.mark.parametrize("cut,force", [("one", ""), ("random", "lzip_round=1"), ("60k", "")])
def test_lzip_sam_bytes_give_the_partials_of_the_text(tmp_path, monkeypatch, grouped, kind, cut, force):
    """The file's bytes pushed whole, cut at random offsets (inside headers, streams and trailers; with lzip_round=1 every push
    is searched and decoded as far as it goes and the rest waits for the next push), or in 60 kB windows."""
    (w, text, skip, o, want), blob = blob_of(tmp_path, grouped, kind)
    cuts = {"one": [], "random": random_cuts(len(blob), 7, 1, 900), "60k": list(range(60_000, len(blob), 60_000))}[cut]
    forced(monkeypatch, force)
    s, got = profile_of(w, grouped, lambda s: s.push_lzip_sam_bytes(blob, skip=skip, cuts=cuts))
    st = s.lzip_stats()
    assert got == want
    assert_matches_oracle(s, o)
    assert_census(st, blob)
    assert 0 < st["max_dist"] <= max(m["data_size"] for m in Z.walk(blob)) and 0 < st["match_bytes"] < len(text), st
    if kind == "d4k":
        assert st["max_dist"] <= 4096 and st["max_dict"] == 4096, st
    if cut == "random" and st["members"] > 1:
        assert st["rounds"] > 1, st
    if cut == "one":
        assert st["rounds"] == 1, st
    s.close()


@pytest.mark.parametrize("force", ["", "lzip_round=1"])
def test_every_accepted_directed_input(tmp_path, monkeypatch, force):
    """Whole, and with a round a push (cuts 1 .. 300 bytes apart): the farthest legal distances, the longest match against
    data_size, the short rep in front of the marker, every DS fraction, an empty member, a legal header inside a payload."""
    (w, text, skip, o, want), (good, _) = directed(tmp_path)
    forced(monkeypatch, force)
    assert sorted(good) == sorted(LD.ACCEPTED)
    for name, (blob, dtext, dskip) in good.items():
        cuts = random_cuts(len(blob), 5, 1, 300) if force else []
        s, got = profile_of(w, True, lambda s: s.push_lzip_sam_bytes(blob, skip=dskip, cuts=cuts))
        st = s.lzip_stats()
        assert got == want, name
        assert_census(st, blob)
        if name == "every_ds_fraction":
            assert st["max_dist"] == 8192 and st["members"] == 9, st   # (the farthest of the eight; the ninth member holds the records)
        if name == "distance_equal_to_the_dictionary":
            assert st["max_dist"] >= 4096, st
        if name == "empty_member_between":
            assert st["empty_members"] == 1, st
        s.close()


def refused_cases(tmp_path):
    c, (_, bad) = directed(tmp_path)
    _, cases = Z.damaged(case(tmp_path, True)[1])
    out = {"damage_" + k: (b, w, False) for k, (b, w) in cases.items()}
    out.update({"directed_" + k: (b, LD.REFUSED[k], True) for k, b in bad.items()})
    return out


REFUSED = ["damage_" + k for k in Z.DAMAGE] + ["directed_" + k for k in sorted(LD.REFUSED)]


@pytest.mark.parametrize("name", REFUSED)
def test_what_is_refused_is_an_error_in_the_host_readers_words_and_the_context_stays_usable(tmp_path, monkeypatch, name):
    """SLIMM_E_INVALID with the words and the named cause, pushed whole and in 300-byte pieces; then slimm_reset and a good
    file on the same context give the right profile."""
    cases = refused_cases(tmp_path)
    assert sorted(cases) == sorted(REFUSED)
    data, word, small = cases[name]
    w, text, skip, o, want = case(tmp_path, True, 50 if small else 1_000)
    forced(monkeypatch, "")
    good = Z.written_copies(text)["three_members"]
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    for kw in (dict(), dict(window=300)):
        with pytest.raises(Exception) as e:
            s.push_lzip_sam_bytes(data, skip=skip, **kw)
        assert WORDS in str(e.value) and word in str(e.value), (name, kw, str(e.value))
        s.reset()
    assert s.push_lzip_sam_bytes(good, skip=skip) == len(w.records)
    s.get_profiles()
    assert integers(s) == want
    assert_matches_oracle(s, o)
    assert_census(s.lzip_stats(), good)
    s.close()


@pytest.mark.parametrize("force,rounds", [("lzip_round_text=27000", 17), ("lzip_round_text=1,lzip_round=1", 17), ("lzip_round_text=60000", 9)])
def test_a_round_takes_the_members_that_fit_and_the_next_round_the_rest(tmp_path, monkeypatch, force, rounds):
    """SLIMM_FORCE lzip_round_text=N: a round ends in front of the member that would take its text past N -- one member alone
    when it is larger --, and the next round starts there.  The 17 members hold 26 222 bytes of text each (the last fewer): a
    member a round below twice that, two a round from there."""
    (w, text, skip, o, want), blob = blob_of(tmp_path, True, "m17")
    forced(monkeypatch, force)
    for cuts in ([], random_cuts(len(blob), 3, 1, 5_000)):
        s, got = profile_of(w, True, lambda s: s.push_lzip_sam_bytes(blob, skip=skip, cuts=cuts))
        st = s.lzip_stats()
        assert got == want
        assert_matches_oracle(s, o)
        assert_census(st, blob)
        assert st["rounds"] == rounds if not cuts else st["rounds"] >= rounds, st
        s.close()


@pytest.mark.parametrize("force", ["", "lzip_round=1"])
def test_last_line_without_newline(tmp_path, monkeypatch, force):
    """The text's last line has no newline: it is a line all the same, in a window of its own -- also when the last push
    carries no byte."""
    w, text, skip, o, _ = case(tmp_path, True, tail_newline=False)
    forced(monkeypatch, force)
    blob = Z.members(text, 30_000)
    for empty_last in (False, True):
        s, _ = profile_of(w, True, lambda s: s.push_lzip_sam_bytes(blob, skip=skip, window=5_000, empty_last=empty_last))
        assert_matches_oracle(s, o)
        s.close()


@pytest.mark.parametrize("force", ["", "lzip_round_text=1,lzip_round=1"])
def test_a_first_member_that_holds_only_part_of_the_header(tmp_path, monkeypatch, force):
    """`skip` reaches across members: the header's first 100 bytes are a member, the next 50 another, then an empty one."""
    w, text, skip, o, want = case(tmp_path, True)
    assert skip > 200
    forced(monkeypatch, force)
    blob = Z.member(text[:100]) + Z.member(text[100:150]) + Z.member(b"") + Z.members(text[150:], 40_000)
    s, got = profile_of(w, True, lambda s: s.push_lzip_sam_bytes(blob, skip=skip, cuts=random_cuts(len(blob), 11, 1, 2_000) if force else []))
    assert got == want
    assert_matches_oracle(s, o)
    assert_census(s.lzip_stats(), blob)
    s.close()


def test_lzip_does_not_mix_with_other_forms_and_is_not_cut_by_byte_range(tmp_path, monkeypatch):
    (w, text, skip, _, _), blob = blob_of(tmp_path, True, "one")
    forced(monkeypatch, "")
    got = C.c_uint64()
    filler = np.zeros(64, dtype=np.uint8)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_lzip_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_sam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 10, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "do not mix" in s.L.slimm_last_error(s.ctx).decode()
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_lzip_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_xz_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 10, 0, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "do not mix" in s.L.slimm_last_error(s.ctx).decode()
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_set_input_mid_file(s.ctx, 0, 1) == SLIMM_OK
    assert s.L.slimm_push_lzip_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "an lzip stream is not cut by byte range" in s.L.slimm_last_error(s.ctx).decode()
    s.close()


@pytest.mark.parametrize("force", ["lzip_round=1", ""])
def test_a_file_that_waited_across_rounds_and_ends_short_is_truncated(tmp_path, monkeypatch, force):
    """The file cut inside a header, a stream, a trailer: pushed in pieces that are decoded as far as they go, then closed -- by
    the last piece or by an empty last push -- it is `truncated`, never a file with fewer records."""
    w, text, skip, _, _ = case(tmp_path, True)
    forced(monkeypatch, force)
    _, cases = Z.damaged(text)
    for name in Z.TRUNCATED:
        data = cases[name][0]
        for cuts in ([len(data) // 2], random_cuts(len(data), 9, 1, 400)):
            for empty_last in (True, False):
                s = Slimm.for_workload(w, device=0, grouped=True)
                s.set_reference_names(w.ref_names)
                with pytest.raises(Exception) as e:
                    s.push_lzip_sam_bytes(data, skip=skip, cuts=cuts, empty_last=empty_last)
                s.close()
                assert WORDS in str(e.value) and "truncated" in str(e.value), (name, cuts[:3], empty_last, str(e.value))


def test_the_backward_index_of_a_file(tmp_path):
    """slimm_host_lzip_members: the members and the text by the trailers alone; an error where the chain does not close on byte 0."""
    (w, text, skip, _, _), blob = blob_of(tmp_path, True, "m17")
    s = Slimm.for_workload(w, device=0, grouped=True)
    n, t = C.c_uint64(), C.c_uint64()
    p = str(tmp_path / "x.sam.lz")
    open(p, "wb").write(blob)
    assert s.L.slimm_host_lzip_members(p.encode(), C.byref(n), C.byref(t)) == SLIMM_OK and (n.value, t.value) == (17, len(text))
    open(p, "wb").write(blob + b"trailing")
    assert s.L.slimm_host_lzip_members(p.encode(), C.byref(n), C.byref(t)) == SLIMM_E_INVALID
    open(p, "wb").write(blob[:-3])
    assert s.L.slimm_host_lzip_members(p.encode(), C.byref(n), C.byref(t)) == SLIMM_E_INVALID
    s.close()
