"""The sampled count of the tile bucketing (slimm_amd/csrc/tile_plan.h): k_tile_count over every S-th slot, capacities from
k_tile_scan, k_tile_fit behind the scatter, and the exact chain behind that when a capacity did not hold -- against the
oracle on every bin, every per-reference column and the profile, and against slimm_get_bucket_sampling for WHICH chain
placed the buckets.

SLIMM_FORCE sample_stride=S makes the small layouts of these tests sample (by themselves they count everything),
fused_scan=0 / scatter_big=0|1 / tile_shift pick the kernels as in tests/test_gpu_scatter_rounds.py, whose hand-made
streams these are: one record per read, so the records in order ARE the targets in order, reference r lies in tile r
(8192 bins) or r / 2 (16 384).

Which slots a sample sees.  Up to 512 slots (393 216 records) every counting workgroup owns two slots, and of a range the
first slot is always sampled: the sample is the EVEN slots, whatever S.  (So no workgroup owns unsampled slots only; the
nearest thing is a range whose sampled slot holds no target -- `sampled_slots_unmapped`.)  Phase B's selectors are dense,
one per mapped read, in pieces of 256 of which every workgroup owns two and samples the first: the even pieces.  `hot`
below marks the records outside both samples.

Capacities: cap(c) = S c + S k^2 / 2 + k S ceil(sqrt(4 c + k^2)) / 2 + S.  At S = 2, k = 8 cap(0) = 130 and cap(50) = 302:
40 000 targets over 8 copies of 49 tiles are about 100 per stretch, so a well-mixed stream fits with room to spare, and
1 600 extra values in one stretch do not.  The cases whose point is a sample that saw NOTHING of a stretch of 50 or 100
values force k = 2 (cap(0) = 10 at S = 2, 20 at S = 4): with k = 8 such a stretch fits by design.
"""
import os
import functools

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from slimm_amd.synth import SynthConfig, make_workload, synth_taxonomy
from slimm_amd.workload import Options, Records, Workload
from tests.helpers import assert_matches_oracle, force

pytestmark = pytest.mark.gpu

N_REFS = 48
REF_LEN = 8_192_000
SLOT = 768
PIECE = 256
N = 40_000


def stream(refs, mapped=None, multi=None, last_tile=None, seed=1, name="hand"):
    """One read per entry of `refs` with one record on that reference; mapped[i] False: the read is unmapped; multi[i]: a
    second record on the next reference (no selector in phase B); last_tile[i]: a position in the reference's last 40
    bins (reference 47: the last tile of the layout at both tile sizes)."""
    refs = np.asarray(refs, dtype=np.int64)
    n = refs.shape[0]
    rng = np.random.Generator(np.random.PCG64(seed))
    mapped = np.ones(n, dtype=bool) if mapped is None else np.asarray(mapped, dtype=bool)
    multi = np.zeros(n, dtype=bool) if multi is None else np.asarray(multi, dtype=bool) & mapped
    last_tile = np.zeros(n, dtype=bool) if last_tile is None else np.asarray(last_tile, dtype=bool)
    reps = 1 + multi.astype(np.int64)
    rd = np.repeat(np.arange(n, dtype=np.int64), reps)
    second = np.concatenate([[False], rd[1:] == rd[:-1]])
    ref = np.where(second, (refs[rd] + 1) % N_REFS, refs[rd])
    pos = np.where(last_tile[rd], rng.integers(8_150_000, 8_190_000, size=rd.shape[0]), rng.integers(0, 4_000_000, size=rd.shape[0]))
    key = (rd.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) & np.uint64((1 << 62) - 1)
    flag = np.where(second, 0x100, 0).astype(np.uint16)
    ref = np.where(mapped[rd], ref, -1)
    pos = np.where(mapped[rd], pos, -1)
    flag = np.where(mapped[rd], flag, 4).astype(np.uint16)
    tax = synth_taxonomy(N_REFS)
    return Workload([a + ".1" for a in tax.accessions], np.full(N_REFS, REF_LEN, dtype=np.uint32), tax,
                    Records(key, flag, ref.astype(np.int32), pos.astype(np.int32)), avg_read_len=100,
                    options=Options(bin_width=1000), name=name)


I = np.arange(N, dtype=np.int64)
MIXED = np.random.Generator(np.random.PCG64(5)).integers(0, N_REFS, size=N)
EVEN_SLOT = (I // SLOT) % 2 == 0
HOT = ~EVEN_SLOT & ((I // PIECE) % 2 == 1)  # records that neither phase's sample sees

# a single tile cut into several work items (the model: HOT_TILE of tests/test_gpu_layouts.py), 260 slots
HOT_TILE = SynthConfig("hot_tile", 200_000, 12, 1.3, bin_width=1000, len_lo=300_000, len_hi=600_000, present_frac=0.5)

FEW = np.concatenate([np.zeros(SLOT, dtype=np.int64), np.arange(100, dtype=np.int64) % N_REFS])
FEW_MAPPED = np.arange(SLOT + 100) >= SLOT

# case: (workload, extra SLIMM_FORCE keys, (stride, fallback) of phase A, of phase B (None: not pinned down), keep_bins)
CASES = {
    "well_mixed": (lambda: stream(MIXED), {}, (2, 0), (2, 0), True),
    # every target outside the samples in ONE tile: its stretches overrun, the exact chain places the buckets
    "hot_unsampled": (lambda: stream(np.where(HOT, 0, MIXED)), {}, (2, 1), (2, 1), True),
    "hot_unsampled_no_bins": (lambda: stream(np.where(HOT, 0, MIXED)), {}, (2, 1), (2, 1), False),
    # no head-room at all: cap = 2 c + 2, which about half of the stretches exceed
    "k0": (lambda: stream(MIXED), {"sample_k": 0}, (2, 1), (2, 1), True),
    # fewer slots than S, the sampled one without a target: the sample sees nothing, cap(0) = 4 * 4 + 4 = 20 at k = 2 -- room
    # for the two or three values a stretch gets when they are spread, not for 100 in one tile
    "fewer_slots_than_S": (lambda: stream(FEW, mapped=FEW_MAPPED), {"sample_stride": 4, "sample_k": 2}, (4, 0), (4, 0), True),
    "fewer_slots_than_S_one_tile": (lambda: stream(np.where(FEW_MAPPED, 5, 0), mapped=FEW_MAPPED),
                                    {"sample_stride": 4, "sample_k": 2}, (4, 1), (4, 0), True),
    "a_handful": (lambda: stream(np.arange(7) % 3), {}, (2, 0), (2, 0), True),
    # every range's sampled slot holds unmapped reads only: all capacities are cap(0) = 10 (k = 2) against ~50 values
    "sampled_slots_unmapped": (lambda: stream(MIXED, mapped=~EVEN_SLOT), {"sample_k": 2}, (2, 1), None, True),
    "empty_tiles": (lambda: stream(np.array([0, 20, 40])[MIXED % 3]), {}, (2, 0), (2, 0), True),
    "hot_tile_split": (lambda: make_workload(HOT_TILE, seed=11), {}, (2, 0), None, True),
    "hot_tile_split_fallback": (lambda: make_workload(HOT_TILE, seed=11), {"sample_k": 0}, (2, 1), None, True),
    # the overrun in the LAST stretch of the buffer: the values outside the samples -- a third of all -- go to the last tile,
    # 1 600 per copy against a capacity of ~300.  The test gives the allocation (bucket_room, LAST_ROOM below) about what the
    # capacities add up to -- 392 stretches of cap(51) = 306 or 200 of cap(100) = 442 --, so the last copy's values run
    # past its end (or, the sum a little above the room, k_tile_scan raises the flag and every base is of no use): either
    # way stores would leave the buffer without the clamp, and either way the exact chain places the buckets
    "last_stretch": (lambda: stream(np.where(HOT, N_REFS - 1, MIXED), last_tile=HOT), {}, (2, 1), (2, 1), True),
    "few_selectors": (lambda: stream(MIXED[: N // 2], multi=(I[: N // 2] % 10) != 0), {}, (2, 0), (2, 0), True),
    "no_selector": (lambda: stream(MIXED[: N // 2], multi=np.ones(N // 2, dtype=bool)), {}, (2, 0), (2, 0), True),
    # an allocation without head-room: the capacities' sum exceeds it and k_tile_scan itself raises the flag
    "caps_above_allocation": (lambda: stream(MIXED), {"bucket_room": N + 1}, (2, 1), (2, 1), True),
    "keep_bins_false": (lambda: stream(MIXED), {}, (2, 0), (2, 0), False),
    "stride_1_forced": (lambda: stream(MIXED), {"sample_stride": 1}, (1, 0), (1, 0), True),
}


LAST_ROOM = {"13": 121_000, "14": 89_500}


@functools.lru_cache(maxsize=None)
def workload_and_oracle(case):
    w = CASES[case][0]()
    assert len(w.records) <= 300_000  # (the host emulator of tests/native runs them too)
    return w, run_workload(w, use_qnames=False)


def profile(monkeypatch, case, **knobs):
    _, extra, _, _, keep = CASES[case]
    force(monkeypatch, **{"sample_stride": 2, **extra, **knobs})
    w, o = workload_and_oracle(case)
    s = Slimm.for_workload(w, device=0)
    if not keep:
        s.keep_bins(False)
    s.push_records(w.records)
    assert s.get_profiles() is not None and not o.no_hits
    assert_matches_oracle(s, o, bins=keep)
    v = s.bucket_sampling()
    print(case, knobs, v)
    return v


@pytest.mark.parametrize("big", ["1", "0"], ids=["ordered_rounds", "direct_rounds"])
@pytest.mark.parametrize("shift", ["13", "14"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_sampled_count(monkeypatch, case, shift, big):
    room = {"bucket_room": LAST_ROOM[shift]} if case == "last_stretch" else {}
    v = profile(monkeypatch, case, fused_scan="0", tile_shift=shift, scatter_big=big, **room)
    for ph, want in (("A", CASES[case][2]), ("B", CASES[case][3])):
        if want is not None:
            assert (v[ph]["stride"], v[ph]["fallback"]) == want, (ph, v)
        assert v[ph]["fallback"] == 0 or v[ph]["stride"] > 1
        if v[ph]["stride"] > 1 and not v[ph]["fallback"]:
            assert v[ph]["peak_1024"] <= 1024


@pytest.mark.parametrize("shift", ["13", "14"])
@pytest.mark.parametrize("case", ["well_mixed", "hot_unsampled"])
def test_fused_layouts_count_everything(monkeypatch, case, shift):
    """The fused kernel scans inside its scatter: the plan keeps S = 1 for it, whatever is forced."""
    v = profile(monkeypatch, case, tile_shift=shift)
    assert v["A"] == {"stride": 1, "fallback": 0, "peak_1024": 0} and v["B"] == v["A"]


LONG_N = 3_200_000  # 4 167 slots: 18 per counting workgroup, waves 0 and 1 have two; 50 pieces of selectors per workgroup


@functools.lru_cache(maxsize=None)
def long_workload_and_oracle():
    w = stream(np.random.Generator(np.random.PCG64(9)).integers(0, N_REFS, size=LONG_N), name="long-ranges")
    return w, run_workload(w, use_qnames=False)


@pytest.mark.parametrize("big", ["1", "0"], ids=["ordered_rounds", "direct_rounds"])
@pytest.mark.parametrize("shift", ["13", "14"])
def test_ranges_of_many_slots(monkeypatch, shift, big):
    """The walk of a sampled count where a wave has several slots (pieces) of its workgroup's range: the first sampled one
    of wave w is w + 16 ((S - w % S) % S) -- at S = 2 wave 1 samples its SECOND slot, number 17 of the range, and not its
    first --, the next S * 16 further (the selectors' pieces 0 and 32 of wave 0).  A well-mixed stream must fit, and the
    fullest stretch says whether the sample was 1 in S: 8 160 (8192-bin tiles) or 16 000 values per stretch have capacities
    of 9 260 and 17 500 at S = 2, k = 8, i.e. 0.88 and 0.91 of them before any deviation -- a sample of 1 in 4 would put
    every stretch above its capacity, one that took every slot near 0.47."""
    if os.environ.get("SLIMM_EMU") == "1":
        pytest.skip("3.2 M records: too many for the host emulator")
    force(monkeypatch, fused_scan="0", tile_shift=shift, scatter_big=big, sample_stride=2)
    w, o = long_workload_and_oracle()
    s = Slimm.for_workload(w, device=0)
    s.push_records(w.records)
    assert s.get_profiles() is not None
    assert_matches_oracle(s, o)
    v = s.bucket_sampling()
    print("long", shift, big, v)
    for ph in "AB":
        assert (v[ph]["stride"], v[ph]["fallback"]) == (2, 0), v
        assert 0.80 * 1024 <= v[ph]["peak_1024"] <= 1024, v


def test_small_layouts_count_everything_by_themselves(monkeypatch):
    """Without sample_stride the plan samples only where a (copy, tile) stretch gets 2048 values or more."""
    force(monkeypatch, fused_scan="0")
    w, o = workload_and_oracle("well_mixed")
    s = Slimm.for_workload(w, device=0)
    s.push_records(w.records)
    assert s.get_profiles() is not None
    assert_matches_oracle(s, o)
    v = s.bucket_sampling()
    assert v["A"]["stride"] == 1 and v["B"]["stride"] == 1


def test_the_streams_are_what_they_claim():
    assert HOT.sum() > N // 4 and not (HOT & EVEN_SLOT).any() and not (HOT & ((I // PIECE) % 2 == 0)).any()
    w = CASES["last_stretch"][0]()
    r = w.records
    nb = (REF_LEN // 1000 + 1 + 3) // 4 * 4  # (every reference's bins padded to a multiple of four)
    gbin = r.ref_id.astype(np.int64) * nb + (r.begin_pos + 50) // 1000
    total = N_REFS * nb
    for shift in (13, 14):
        assert ((gbin[HOT] >> shift) == ((total - 1) >> shift)).all()
    w = CASES["sampled_slots_unmapped"][0]()
    assert (w.records.ref_id[EVEN_SLOT] < 0).all() and (w.records.ref_id[~EVEN_SLOT] >= 0).all()
