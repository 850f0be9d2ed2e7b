"""The rounds of the bucket scatter that order their values by tile in LDS (k_tile_scatter_big) against the oracle, on
inputs built for what a round does: one LDS add per value whose result is the value's rank inside its tile, runs of
equal tiles, lanes and rounds that are partly or wholly empty, and the dense form of phase B.

SLIMM_FORCE fused_scan=0 sends small layouts through k_tile_scan + k_tile_scatter_big, tile_shift picks the tile size;
every case runs with scatter_big=0 (the direct rounds) as well, and both must give the oracle's numbers.

The streams are hand-made: a read with ONE record is one target, so a list of (reference, position) per read IS the
target stream in order.  Every reference is 8 192 000 bases long at a bin width of 1000: 8193 bins, so reference r
begins about r tiles of 8192 bins (r / 2 tiles of 16 384) into the layout, and positions below 4 000 000 stay inside
that tile.  Inputs stay below 300 K records so that the host emulator (tests/native) runs them too.
"""
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
STEP = 4            # references this far apart lie in different tiles at both tile sizes
ROUND = 1024 * 24   # values of one round of a workgroup
WAVE_ROUND = 6 * 256  # ... of one wave in it


def stream(refs, multi=None, seed=1, name="hand"):
    """One read per entry of `refs`, one record on that reference (a target each).  multi: a boolean per read -- these
    reads get a second record on reference (r + 1) % N_REFS, which makes them multi-mapped (no selector in phase B)."""
    refs = np.asarray(refs, dtype=np.int64)
    n = refs.shape[0]
    rng = np.random.Generator(np.random.PCG64(seed))
    multi = np.zeros(n, dtype=bool) if multi is None else np.asarray(multi, dtype=bool)
    reps = 1 + multi.astype(np.int64)
    rd = np.repeat(np.arange(n, dtype=np.int64), reps)
    second = np.concatenate([[False], rd[1:] == rd[:-1]])
    ref = np.where(second, (refs[rd] + 1) % N_REFS, refs[rd])
    pos = rng.integers(0, 4_000_000, size=rd.shape[0])
    key = (rd.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) & np.uint64((1 << 62) - 1)
    flag = np.where(second, 0x100, 0).astype(np.uint16)
    tax = synth_taxonomy(N_REFS)
    return Workload([a + ".1" for a in tax.accessions], np.full(N_REFS, REF_LEN, dtype=np.uint32), tax,
                    Records(key, flag, ref.astype(np.int32), pos.astype(np.int32)), avg_read_len=100,
                    options=Options(bin_width=1000), name=name)


def runs(lengths, n):
    """n targets in runs of equal tiles: run i has lengths[i % len(lengths)] targets on reference (i * STEP) % N_REFS"""
    lengths = np.asarray(lengths, dtype=np.int64)
    k = int(n // lengths.mean()) + len(lengths) + 1
    ln = lengths[np.arange(k) % len(lengths)]
    return np.repeat((np.arange(k, dtype=np.int64) * STEP) % N_REFS, ln)[:n]


def long_reads_workload(hits, seed=41):
    """Reads with `hits` targets each (as many different references, two to three bins long: ~80 tiles of 8192 bins) in
    front of a stream of short reads: one slot's values fill a wave's share of several rounds."""
    base = make_workload(SynthConfig("many-refs", 20_000, 40_000, 2.0, bin_width=100, len_lo=1_500, len_hi=3_000,
                                     present_frac=0.5), seed=seed)
    r = base.records
    parts = []
    for j, h in enumerate(hits):
        parts.append(Records(np.full(h, int(r.read_key.max()) + 1 + j, dtype=np.uint64),
                             np.where(np.arange(h) > 0, 0x100, 0).astype(np.uint16),
                             ((np.arange(h, dtype=np.int64) * 7 + j) % 40_000).astype(np.int32), np.full(h, 10, dtype=np.int32)))
    parts.append(r)
    rec = Records(*(np.concatenate([getattr(x, f) for x in parts]) for f in ("read_key", "flag", "ref_id", "begin_pos")))
    return Workload(base.ref_names, base.ref_len, base.taxonomy, rec, base.avg_read_len, base.options, "long-reads")


# a single tile cut into several work items (the model: HOT_TILE of tests/test_gpu_layouts.py)
HOT_TILE = SynthConfig("hot_tile", 300_000, 12, 1.3, bin_width=1000, len_lo=300_000, len_hi=600_000, present_frac=0.5)


def _cases():
    n = 60_000
    i = np.arange(n, dtype=np.int64)
    rng = np.random.Generator(np.random.PCG64(77))
    c = {
        "one_tile": lambda: stream(np.zeros(n)),
        "two_tiles_alternating": lambda: stream((i & 1) * STEP),
        "quads_equal": lambda: stream(((i // 4) * STEP) % N_REFS),
        "quads_all_different": lambda: stream((i * STEP) % N_REFS),
        # runs that end inside a lane's four values, cross lanes, a piece of 256 values, and slots (a slot's targets are a
        # few hundred: runs of 1000 and 5000 cross several)
        "runs_across_lanes": lambda: stream(runs([1, 2, 3, 5, 6, 7, 9], n)),
        "runs_across_pieces": lambda: stream(runs([255, 256, 257, 300, 64, 63, 65], n)),
        "runs_across_slots": lambda: stream(runs([1000, 5000, 1, 777, 2049], n)),
        "random_tiles": lambda: stream(rng.integers(0, N_REFS, size=n)),
        "less_than_a_round": lambda: stream(runs([3, 1, 4, 1, 5], ROUND - 1)),
        "exactly_a_round": lambda: stream(runs([3, 1, 4, 1, 5], ROUND)),
        "a_round_and_one": lambda: stream(runs([3, 1, 4, 1, 5], ROUND + 1)),
        "a_handful": lambda: stream(runs([2, 1], 7)),
        # slots without a target: stretches of thousands of unmapped reads between the mapped ones
        "slots_without_targets": lambda: _with_unmapped(stream(runs([3, 1, 4, 1, 5], n)), 5_000, 12_000),
        # phase B: nine reads of ten are multi-mapped and have no selector
        "few_selectors": lambda: stream(runs([1, 2, 3, 5], n), multi=(i % 10) != 0),
        "no_selector_at_all": lambda: stream(runs([1, 2, 3, 5], 20_000), multi=np.ones(20_000, dtype=bool)),
        # one slot's values over a wave's share of one round less one, one round, one more, and of many rounds
        "long_reads": lambda: long_reads_workload([WAVE_ROUND - 1, WAVE_ROUND, WAVE_ROUND + 1, 30_000]),
        "hot_tile": lambda: make_workload(HOT_TILE, seed=11),
    }
    return c


def _with_unmapped(w, every, length):
    """`length` unmapped reads after every `every` reads of w"""
    r = w.records
    n = len(r)
    parts = []
    key0 = np.uint64(1) << np.uint64(61)
    for a in range(0, n, every):
        parts.append(r.take(np.arange(a, min(a + every, n))))
        k = key0 + np.arange(a * 4, a * 4 + length, dtype=np.uint64)
        parts.append(Records(k, np.full(length, 4, dtype=np.uint16), np.full(length, -1, dtype=np.int32),
                             np.full(length, -1, dtype=np.int32)))
    rec = Records(*(np.concatenate([getattr(x, f) for x in parts]) for f in ("read_key", "flag", "ref_id", "begin_pos")))
    return Workload(w.ref_names, w.ref_len, w.taxonomy, rec, w.avg_read_len, w.options, w.name + "-unmapped")


CASES = _cases()


@pytest.mark.parametrize("big", ["1", "0"], ids=["ordered_rounds", "direct_rounds"])
@pytest.mark.parametrize("shift", ["13", "14"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_scatter_rounds(monkeypatch, case, shift, big):
    force(monkeypatch, fused_scan="0", tile_shift=shift, scatter_big=big)
    w = CASES[case]()
    assert len(w.records) <= 300_000
    o = run_workload(w, use_qnames=False)
    s = Slimm.for_workload(w, device=0)
    s.push_records(w.records)
    assert s.get_profiles() is not None and not o.no_hits
    assert_matches_oracle(s, o)
    if case == "hot_tile":
        assert s.stats()["n_targets"] > 20 * s.stats()["total_bins"] / 8192  # far more than a work item's worth in one tile


def test_the_hand_made_streams_are_what_they_claim():
    """The tiles of the targets, computed as the library computes them, for the cases whose point is a pattern of tiles."""
    def tiles(w, shift):
        r = w.records
        nb = w.ref_len.astype(np.int64) // 1000 + 1
        off = np.concatenate([[0], np.cumsum(nb)])
        first = np.concatenate([[True], r.read_key[1:] != r.read_key[:-1]])
        m = first & (r.ref_id >= 0)
        return (off[r.ref_id[m]] + (r.begin_pos[m] + 50) // 1000) >> shift
    for shift in (13, 14):
        assert np.unique(tiles(CASES["one_tile"](), shift)).size == 1
        t = tiles(CASES["two_tiles_alternating"](), shift)
        assert np.unique(t).size == 2 and (t[1:] != t[:-1]).all()
        q = tiles(CASES["quads_equal"](), shift).reshape(-1, 4)
        assert (q == q[:, :1]).all() and (q[1:, 0] != q[:-1, 0]).all()
        q = tiles(CASES["quads_all_different"](), shift).reshape(-1, 4)
        assert all(np.unique(row).size == 4 for row in q[:64])
        assert np.unique(tiles(CASES["random_tiles"](), shift)).size >= N_REFS // 2
