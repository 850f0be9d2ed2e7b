"""k_filter_compact against the oracle on slots built for its edges: chunks of 64 targets, batches of 256 (a slot's last one
may be partial), a ring of 128 valid entries drained 64 at a time in windows of whole reads, reads of 64 valid targets and
more (left to k_filter_walk), reads that keep no target, and reads on whose targets no level agrees (quirk Q4).

The streams are hand-made.  A slot is 768 consecutive records; the reads that START in it are its reads, a mapped record
is a target (every read here names a reference once), an unmapped record is a read of its own without a target -- so the
number of mapped records in a slot is its number of targets, and every hand-made slot is filled up to 768 records with
unmapped ones.

Which targets are VALID is decided by the coverage cut-offs (the quantile of cov_pct / ucov_pct over the references with
a unique read; a reference is valid at or above both).  The "good" references are 8500 bases long -- nine bins of 1000 --
and a preamble of two one-record reads per bin gives each of them cov_pct = ucov_pct = 1; the "bad" ones are 8 192 000
bases long and every record on them lies in one bin (1 / 8193).  Both cut-offs come out as 1: good references are valid,
bad ones are not, whatever else the case adds.  Every case asserts that from the oracle's result before it compares.
Eight of the good references have a lineage of their own up to the superkingdom: a read on one of them and on one of
the others agrees at no level (Q4).

Inputs stay far below 300 K records so that the host emulator (tests/native, SLIMM_EMU=1) runs them too.
"""
import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from slimm_amd.workload import RANKS, Options, Records, Taxonomy, Workload
from tests.helpers import assert_matches_oracle, force

pytestmark = pytest.mark.gpu

SLOT = 768
N_GOOD, N_ARCH, N_BAD = 80, 8, 16     # good: references 0..79, the last N_ARCH of them with a lineage of their own
N_REFS = N_GOOD + N_BAD
GOOD = np.arange(N_GOOD)
BACT = np.arange(N_GOOD - N_ARCH)
ARCH = np.arange(N_GOOD - N_ARCH, N_GOOD)
BAD = np.arange(N_GOOD, N_REFS)
GOOD_LEN, BAD_LEN, BIN = 8_500, 8_192_000, 1000


def taxonomy():
    """synth_taxonomy's tree (2 references per species, 10 per genus ...), the ARCH references moved into a far corner
    of it: their columns differ from everybody else's at every level, the superkingdom included"""
    i = np.arange(N_REFS, dtype=np.int64)
    i = np.where((i >= ARCH[0]) & (i <= ARCH[-1]), i + 6000, i)
    lin = np.stack([10_000_000 + i, 1_000_000 + i // 2, 500_000 + i // 10, 200_000 + i // 50, 100_000 + i // 200,
                    50_000 + i // 1000, 10_000 + i // 2000, np.where((i // 2000) % 4 == 3, 2157, 2)], axis=1).astype(np.uint32)
    tid, rk = [], []
    for lv in range(7, -1, -1):
        col = np.unique(lin[:, lv])
        tid.append(col)
        rk.append(np.full(col.shape, lv, dtype=np.uint32))
    tid, rk = np.concatenate(tid), np.concatenate(rk)
    return Taxonomy([f"ACC{k:06d}" for k in range(N_REFS)], lin, tid, rk,
                    [f"{RANKS[r]}_{t}" for t, r in zip(tid.tolist(), rk.tolist())])


class Stream:
    """Records of whole reads, slot by slot."""

    def __init__(self, seed):
        self.key, self.flag, self.ref, self.pos = [], [], [], []
        self.reads = 0
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.targets = []   # reference of every target, in order
        self.heads = []     # ... and whether it is its read's first

    def _key(self):
        self.reads += 1
        return (self.reads * 0x9E3779B97F4A7C15) & ((1 << 62) - 1)

    def read(self, refs, pos=10, key=None, mate=0):
        """one read with a record on each of `refs` (all different); no reference: an unmapped record"""
        refs = list(refs)
        assert len(set(refs)) == len(refs)
        key = self._key() if key is None else key
        if not refs:
            self.key.append(key), self.flag.append(4 | mate), self.ref.append(-1), self.pos.append(-1)
        for k, r in enumerate(refs):
            self.key.append(key), self.flag.append(mate | (0x100 if k else 0)), self.ref.append(int(r)), self.pos.append(pos)
            self.targets.append(int(r)), self.heads.append(k == 0)
        return key

    def fill(self):
        """unmapped records up to the slot's end"""
        while len(self.key) % SLOT:
            self.read([])

    def slot(self, reads):
        """a slot of its own with these reads"""
        assert len(self.key) % SLOT == 0
        n0 = len(self.key)
        for r in reads:
            self.read(r)
        assert len(self.key) - n0 <= SLOT, "more records than a slot holds"
        self.fill()

    def preamble(self, refs=GOOD):
        """two unique reads in every bin of the good references: cov_pct = ucov_pct = 1"""
        for r in refs:
            for b in range(GOOD_LEN // BIN + 1):
                self.read([r], pos=b * BIN)
                self.read([r], pos=b * BIN + 5)
        self.fill()

    def ordinary(self, good=0.5, n_reads=250):
        """a slot of short reads on good and bad references"""
        self.slot(self.short_reads(n_reads * 2, good)[:n_reads])

    def short_reads(self, n_targets, good=0.5, lengths=(1, 2, 3, 1, 5)):
        """reads of a few targets each, n_targets in all, a target on a good reference with probability `good`"""
        out, k = [], 0
        while n_targets:
            n = min(lengths[k % len(lengths)], n_targets)
            k += 1
            g = self.rng.random(n) < good
            refs = np.where(g, self.rng.permutation(BACT)[:n], self.rng.permutation(BAD)[:n])
            out.append(refs.tolist())
            n_targets -= n
        return out

    def pattern_reads(self, valid, lengths=(1, 2, 3)):
        """reads over the targets valid[0], valid[1] ...: True = a good reference, False = a bad one"""
        out, i, k = [], 0, 0
        gi = bi = 0
        while i < len(valid):
            n = min(lengths[k % len(lengths)], len(valid) - i)
            k += 1
            refs = []
            for v in valid[i:i + n]:
                if v:
                    refs.append(int(BACT[gi % len(BACT)]))
                    gi += 1
                else:
                    refs.append(int(BAD[bi % len(BAD)]))
                    bi += 1
            assert len(set(refs)) == n
            out.append(refs)
            i += n
        return out

    def workload(self, name, cov_cut_off=0.95):
        rec = Records(np.array(self.key, dtype=np.uint64), np.array(self.flag, dtype=np.uint16),
                      np.array(self.ref, dtype=np.int32), np.array(self.pos, dtype=np.int32))
        tax = taxonomy()
        ref_len = np.where(np.arange(N_REFS) < N_GOOD, GOOD_LEN, BAD_LEN).astype(np.uint32)
        return Workload([a + ".1" for a in tax.accessions], ref_len, tax, rec, avg_read_len=100,
                        options=Options(bin_width=BIN, cov_cut_off=cov_cut_off), name=name)


def spread(n, k):
    """n flags, k of them set, evenly"""
    v = np.zeros(n, dtype=bool)
    v[(np.arange(k) * n) // max(k, 1)] = True
    assert v.sum() == k
    return v


def singles(n, first=0):
    """n reads of one valid target each"""
    return [[int(BACT[(first + k) % len(BACT)])] for k in range(n)]


def valid_run(n, first=0):
    """n different good references (a read of n valid targets)"""
    assert n <= N_GOOD - N_ARCH
    return [int(BACT[(first + k) % len(BACT)]) for k in range(n)]


# ---- the cases: (stream, what the oracle must say about validity) ----
def case_slot_sizes():
    """slots of 0 ... 513 targets -- chunk and batch edges -- each followed by an ordinary slot"""
    s = Stream(1)
    s.preamble()
    for t in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513):
        s.slot(s.short_reads(t))
        s.ordinary()
    return s, "mix"


def case_valid_counts():
    """63 ... 129 valid entries in a slot of 400 targets: the ring wraps, 63 entries left over meet 64 new ones"""
    s = Stream(2)
    s.preamble()
    for v in (63, 64, 65, 127, 128, 129):
        s.slot(s.pattern_reads(spread(400, v)))
        s.ordinary()
    # ... and the same counts packed: every target valid up to the count, nothing valid behind it
    for v in (63, 64, 65, 127, 128, 129):
        s.slot(s.pattern_reads(np.arange(300) < v))
    return s, "mix"


def case_alternating():
    """valid and invalid targets alternating lane by lane, in phase and out of phase with the reads' boundaries"""
    s = Stream(3)
    s.preamble()
    lane = np.arange(513)
    s.slot(s.pattern_reads(lane % 2 == 0))
    s.slot(s.pattern_reads(lane % 2 == 1, lengths=(2,)))
    s.slot(s.pattern_reads(lane[:257] % 2 == 0, lengths=(3, 1)))
    s.slot(s.pattern_reads(lane[:768] % 2 == 1, lengths=(1,)))
    s.ordinary()
    return s, "mix"


def case_all_valid():
    """every target valid: every chunk fills a window"""
    s = Stream(4)
    s.preamble()
    for t in (300, 768, 257, 64, 128):
        s.slot(s.pattern_reads(np.ones(t, dtype=bool)))
    s.slot(s.pattern_reads(np.ones(SLOT, dtype=bool), lengths=(1,)))
    return s, "all"


def case_none_valid():
    """No reference valid.  Two references have every bin covered but one unique read, two others unique reads in five
    of nine bins: with a quantile of 0.3 the coverage cut-off is 1 and the unique coverage cut-off 5 / 9, and each pair
    fails one of them."""
    s = Stream(5)
    a1, a2, b1, b2 = 0, 1, 2, 3
    for b in range(GOOD_LEN // BIN + 1):
        s.read([a1, a2], pos=b * BIN)
    s.read([a1]), s.read([a2])
    for b in range(5):
        s.read([b1], pos=b * BIN), s.read([b2], pos=b * BIN)
    s.fill()
    refs = [a1, a2, b1, b2]
    for t in (300, 513, 64):
        reads, k = [], 0
        while t:
            n = min((1, 2, 3, 4)[k % 4], t)
            reads.append([refs[(k + j) % 4] for j in range(n)])
            k, t = k + 1, t - n
        s.slot(reads)
    return s, "none"


def case_reads_across_edges():
    """reads whose valid targets straddle a chunk's edge, a batch's edge, and the end of a full window"""
    s = Stream(6)
    s.preamble()
    # all valid: targets 62..66 are one read (chunk edge, and the window of the first 64 entries ends inside it), so are
    # 254..258 (batch edge)
    s.slot(singles(62) + [valid_run(5, 3)] + singles(254 - 67, 9) + [valid_run(5, 20)] + singles(40, 5))
    # one target in four valid: the read that holds valid entries 62..66 lies on targets 251..257, across the batch's edge
    s.slot(s.pattern_reads(spread(251, 62)) + [[int(BAD[0])] + valid_run(3, 1) + [int(BAD[1])] + valid_run(2, 30)] + s.pattern_reads(spread(200, 70)))
    # a read of 40 valid targets behind 40 single ones: the first window stops in front of it, the second holds it whole
    s.slot(singles(40) + [valid_run(40, 7)] + singles(30, 50))
    # ... and reads of 33 valid targets one after the other: every window holds one of them
    s.slot([valid_run(33, 5 * k) for k in range(9)])
    s.ordinary()
    return s, "mix"


def case_long_reads():
    """reads of 62 ... 65 valid targets: 64 and more do not fit a window, their slot goes through k_filter_walk"""
    s = Stream(7)
    s.preamble()
    for n in (62, 63, 64, 65):
        # alone among short reads, then with invalid targets between its valid ones and at a batch's edge
        s.slot(s.short_reads(100) + [valid_run(n, n)] + s.short_reads(150))
        s.ordinary()
        mixed = []
        for k, r in enumerate(valid_run(n, 2 * n)):
            mixed.append(r)
            if k % 8 == 0:
                mixed.append(int(BAD[(k // 8) % N_BAD]))
        s.slot(s.short_reads(220) + [mixed] + s.short_reads(60))
        s.ordinary()
    return s, "mix"


def case_reads_without_valid_target():
    """reads that keep no target: a slot's first, its last, runs of them; 768 one-record reads; reads beyond 768"""
    s = Stream(8)
    s.preamble()
    bad = lambda n, k=0: [int(BAD[(k + j) % N_BAD]) for j in range(n)]   # noqa: E731
    s.slot([bad(3)] + s.short_reads(200) + [bad(2, 5)])
    s.slot([bad(1)] + [bad(1 + k % 3, k) for k in range(30)] + [valid_run(2)] + [bad(2, k) for k in range(70)]
           + [valid_run(1, 9), valid_run(3, 11)] + [bad(1, k) for k in range(100)] + [valid_run(2, 40)] + [bad(4)])
    s.ordinary()
    # 768 one-record reads: as many selectors as a slot of whole one-read runs can have
    s.slot([[int(BAD[k % N_BAD])] if k % 3 else [int(BACT[k % len(BACT)])] for k in range(SLOT)])
    # 767 one-record reads and a run of two mates that starts on the slot's last record: 769 reads start in the slot
    for k in range(SLOT - 1):
        s.read([int(BACT[k % len(BACT)])] if k % 5 == 0 else [int(BAD[k % N_BAD])])
    key = s.read([int(BACT[7])], mate=0x41)
    s.read([int(BACT[8]), int(BAD[2])], key=key, mate=0x81)
    s.fill()
    s.ordinary()
    return s, "mix"


def case_q4():
    """reads on whose valid targets no level agrees, in a full batch and in a slot's partial last batch"""
    s = Stream(9)
    s.preamble()
    q4 = lambda k: [int(BACT[k]), int(ARCH[k % N_ARCH])]   # noqa: E731
    s.slot(s.short_reads(40) + [q4(1)] + s.short_reads(100) + [q4(2) + [int(BAD[0]), int(ARCH[5])]] + s.short_reads(300))   # 448 targets
    s.slot(s.short_reads(30) + [q4(3)] + s.short_reads(20))                                          # one partial batch
    s.slot(s.short_reads(256) + [q4(4), [int(ARCH[0]), int(ARCH[1])], q4(5)] + s.short_reads(30))    # full batch + partial one
    s.ordinary()
    return s, "mix"


CASES = {f.__name__[5:]: f for f in (case_slot_sizes, case_valid_counts, case_alternating, case_all_valid, case_none_valid,
                                     case_reads_across_edges, case_long_reads, case_reads_without_valid_target, case_q4)}
_built = {}


def built(case):
    """the case's workload and the oracle's result, computed once and shared by the row forms"""
    if case not in _built:
        s, mix = CASES[case]()
        w = s.workload(case, cov_cut_off=0.3 if mix == "none" else 0.95)
        assert len(w.records) <= 300_000 and len(w.records) % SLOT == 0
        _built[case] = (s, mix, w, run_workload(w, use_qnames=False))
    return _built[case]


@pytest.mark.parametrize("rows", ["rows16", "rows32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_filter_batches(monkeypatch, case, rows):
    if rows == "rows32":
        force(monkeypatch, wide_rows=1)
    s, mix, w, o = built(case)
    # the case holds the mix it was built for
    n_valid, n_with_reads = o.scalars["n_valid"], o.scalars["reference_count"]
    used = np.zeros(N_REFS, dtype=bool)
    used[np.array(s.targets)] = True
    assert n_with_reads == used.sum()
    if mix == "mix":
        assert 0 < n_valid < n_with_reads
        assert o.valid[GOOD].all() and not o.valid[BAD].any() and used[GOOD].all() and used[BAD].any()
    elif mix == "all":
        assert n_valid == n_with_reads == N_GOOD and not used[BAD].any()
    else:
        assert n_valid == 0 and n_with_reads == 4
    lin = w.lineage()
    q4 = [(t, r) for t, r in o.lca_direct_children if t not in lin[r].tolist()]
    assert bool(q4) == (case == "q4"), "reads on whose targets no level agrees: only where they are meant"

    g = Slimm.for_workload(w, device=0)
    g.push_records(w.records)
    assert g.get_profiles() is not None and not o.no_hits
    # the targets are the mapped records, read by read
    ref, _ = g.read_targets()
    assert np.array_equal(ref & 0x7fffffff, np.array(s.targets, dtype=np.uint32))
    assert np.array_equal((ref >> 31) != 0, np.array(s.heads))
    assert_matches_oracle(g, o)
