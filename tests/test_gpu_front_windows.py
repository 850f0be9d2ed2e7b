"""k_front's windows (slimm_amd/csrc/front.hip) on streams built record by record for the window code's edges: segments at
every length at which the duplicate walk changes its form (1, 2, 5, 6, 7, 12, 13), on both sides of the hash-table threshold
(31, 32, 33) and of the hand-over to the long-run path (63, 64, 65); runs that end on a window's last lane, that straddle the
slot's end (records 767 / 768) and the end of the staged stretch (831 / 832); streams that end inside a window; mates 0 / 1 / 2
in order and interleaved; unmapped records at a run's start, middle and end; repeated references next to each other and at the
two ends of a segment, and at every distance up to the threshold; a read whose one target sits on the window's last lane.

A window is up to 64 records from a qName run's start to the last run start among them, so a run followed by a run of 63
records has a window to itself, and short runs in a row share one.  A slot is 768 records, 64 more are staged with it.

Every case goes through the four-array, the packed and the run-marked records and through a context created for
SLIMM_ORDER_ANY, and is checked twice: everything against the oracle, and the target list (slimm_get_read_targets) against
the order the head of front.hip states, restated here in a dozen lines -- per qName run the mates ascending, per read the first
record of every reference in file order, the head bit on a read's first target, the unique bit where it is the only one.

At most four slots and 16 references per stream: the host emulator (tests/native, SLIMM_EMU=1) runs the file in seconds.
"""
import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from slimm_amd.synth import synth_taxonomy
from slimm_amd.workload import Options, Records, Workload
from tests.helpers import assert_matches_oracle

pytestmark = pytest.mark.gpu

SLOT, STAGED = 768, 832
N_REFS = 16
REF_LEN = np.array([900 + 700 * (k % 5) + 13 * k for k in range(N_REFS)], dtype=np.uint32)
BIN, READ_LEN = 100, 100
LENGTHS = (1, 2, 5, 6, 7, 12, 13, 31, 32, 33, 63, 64, 65)
MATE_FLAG = {0: 0, 1: 0x40, 2: 0x80}


class Stream:
    """Records one by one: run() = one qName, a list of (mate, reference or None, position)."""

    def __init__(self):
        self.key, self.flag, self.ref, self.pos = [], [], [], []
        self.runs = self.unmapped = 0

    def __len__(self):
        return len(self.key)

    def run(self, recs):
        self.runs += 1
        key = (self.runs * 0x9E3779B97F4A7C15) & ((1 << 61) - 1)
        for k, (mate, ref, pos) in enumerate(recs):
            unmapped = ref is None
            # (an unmapped record says so by its flag or by its reference, src/slimm.hpp:197: one of each in turn)
            self.unmapped += unmapped
            by_flag = unmapped and self.unmapped % 2 == 0
            self.key.append(key)
            self.flag.append(MATE_FLAG[mate] | (4 if by_flag else 0) | (0x100 if k else 0))
            self.ref.append(-1 if unmapped and not by_flag else (3 if unmapped else int(ref)))
            self.pos.append(-1 if unmapped and not by_flag else int(pos))

    def seg(self, n, mate=0, first=0, step=5):
        """n records of one mate: the references first, first + step ... round the table (step 5 on 16 references: a
        reference comes back after 16 records), every record at a position of its own"""
        return [(mate, (first + step * k) % N_REFS, (41 * (len(self.key) + k) + 7 * mate) % 2500) for k in range(n)]

    def shorts(self, n_records, lengths=(1, 2, 3, 1, 4)):
        """runs of a few records, n_records in all"""
        k = 0
        while n_records:
            n = min(lengths[k % len(lengths)], n_records)
            self.run(self.seg(n, first=k))
            n_records -= n
            k += 1

    def upto(self, at):
        """short runs up to record `at`"""
        assert len(self) <= at
        self.shorts(at - len(self))

    def workload(self, name, n=None):
        n = len(self) if n is None else n
        rec = Records(np.array(self.key[:n], dtype=np.uint64), np.array(self.flag[:n], dtype=np.uint16),
                      np.array(self.ref[:n], dtype=np.int32), np.array(self.pos[:n], dtype=np.int32))
        tax = synth_taxonomy(N_REFS)
        return Workload([a + ".1" for a in tax.accessions], REF_LEN, tax, rec, avg_read_len=READ_LEN,
                        options=Options(bin_width=BIN), name=name)


# ---------------------------------------------------------------------------------------------------------- the cases
def case_length(n):
    """a segment of n records with a window to itself (a run of 63 behind it), then among short runs in one window, then as
    mate 1 of a run whose mate 2 has two records, then with the records of mate 2 in front of it in another run (n < 64:
    a window; else the long path)"""
    def build():
        s = Stream()
        s.run(s.seg(n))
        s.run(s.seg(63, first=1))
        s.run(s.seg(1)), s.run(s.seg(2, first=4))
        s.run(s.seg(n, first=2, step=3))
        s.run(s.seg(1, first=9)), s.run(s.seg(3, first=6))
        s.run(s.seg(63, first=2))
        s.run(s.seg(n, mate=1, first=3) + s.seg(2, mate=2, first=3))
        s.run(s.seg(2, first=7))
        s.run(s.seg(2, mate=0, first=5) + s.seg(n, mate=2, first=5, step=7))
        s.shorts(40)
        return s
    return build


def case_run_ends_on_lane_63():
    """runs of 10 + 20 + 30 + 4 records: the last one ends on lane 63 of the window that starts with the first -- and of
    the window that starts with the second, with one run more behind it"""
    s = Stream()
    for n in (10, 20, 30, 4, 10, 5, 64 - 39, 3, 61, 1, 1, 1):
        s.run(s.seg(n, first=n))
    s.shorts(70)
    return s


def case_slot_end():
    """runs across records 767 / 768: one of 20 records that starts at 760, one that starts ON record 767, and the next
    slot beginning inside a run"""
    s = Stream()
    s.upto(760)
    s.run(s.seg(20, first=2))                  # 760 .. 779
    s.upto(SLOT + 767)
    s.run(s.seg(33, mate=1, first=1) + s.seg(7, mate=2, first=4))   # starts on the second slot's last record
    s.upto(2 * SLOT + 700)
    s.run(s.seg(63, first=8))                  # 2236 .. 2298: the hash path at the slot's end
    s.run(s.seg(40, first=3))                  # 2299 .. 2338 across the end of the third slot
    s.shorts(30)
    return s


def case_staged_end():
    """runs across records 831 / 832, the end of what the first slot stages: one that belongs to the second slot (it starts
    at 800), and in a second stream one of 100 records that starts at 760 -- the first slot's, and longer than its stage"""
    s = Stream()
    s.upto(767)
    s.run(s.seg(33, first=5))                  # 767 .. 799: a window that starts on the slot's last record
    s.run(s.seg(50, first=6))                  # 800 .. 849
    s.shorts(100)
    return s


def case_long_run_past_the_stage():
    s = Stream()
    s.upto(760)
    s.run(s.seg(60, mate=1, first=1) + s.seg(40, mate=2, first=2))    # 760 .. 859
    s.shorts(90)
    s.run(s.seg(70, first=3))                  # a long run inside the second slot's stage
    s.shorts(20)
    return s


def case_sizes():
    """the stream cut at N = 1, 64, 768, 769 and 833 records, and inside a window (100, 1000)"""
    s = Stream()
    s.shorts(40, lengths=(1, 3, 2, 7))
    s.run(s.seg(30, first=4))                  # 40 .. 69: N = 64 cuts it
    s.upto(750)
    s.run(s.seg(25, first=2))                  # 750 .. 774: N = 768 and 769 cut it
    s.upto(820)
    s.run(s.seg(20, first=9))                  # 820 .. 839: N = 833 cuts it
    s.shorts(200)
    return s


SIZES = (1, 64, 100, 768, 769, 833, 1000)


def case_mates():
    """mates 0 / 1 / 2 in order (segments of one run), and interleaved (the general path), short and at 30 records a mate"""
    s = Stream()
    s.run(s.seg(3, 0) + s.seg(4, 1, first=1) + s.seg(2, 2, first=1))
    s.run(s.seg(1, 1) + s.seg(1, 2))
    s.run(s.seg(2, 2, first=3))
    s.run([(1, 2, 10), (2, 2, 700), (1, 3, 20), (2, 5, 30), (1, 2, 40), (0, 7, 50), (2, 2, 60)])      # interleaved
    s.run(s.seg(2))
    s.run([(2, 1, 10), (1, 1, 500)])                                                                    # decreasing
    s.run([(m % 2 + 1, (3 * k) % N_REFS, 17 * k) for k, m in enumerate(range(60))])                    # 30 + 30, alternating
    s.run(s.seg(30, 1, first=2) + s.seg(31, 2, first=2))
    s.run([(2 - k % 3, (k * 5) % N_REFS, 9 * k) for k in range(66)])                                   # interleaved, long path
    s.shorts(50)
    return s


def case_unmapped():
    """unmapped records at a run's start, middle and end; runs and segments without a mapped record"""
    s = Stream()
    u = lambda m=0: (m, None, 0)   # noqa: E731
    s.run([u()] + s.seg(3, first=1))
    s.run(s.seg(2, first=2) + [u(), u()] + s.seg(2, first=8))
    s.run(s.seg(4, first=3) + [u()])
    s.run([u()])
    s.run([u(1), u(1)] + s.seg(2, 2, first=4))
    s.run(s.seg(2, 1, first=4) + [u(2)])
    s.run([u(1)] + s.seg(1, 1, first=6) + [u(1), u(2), u(2)] + s.seg(1, 2, first=6) + [u(2)])
    s.run([u(), u(), u()])
    s.run([u()] + s.seg(20, first=1) + [u()] * 5 + s.seg(10, first=2) + [u()])        # 37 records: the hash path
    s.run([u()] * 40 + s.seg(30, first=7))                                             # 70 records: the long path
    s.shorts(30)
    return s


def case_repeats():
    """the same reference twice in a read: next to each other, and on the first and last record of a segment of L records
    (L = 2, 6, 7, 13, 14, 33, 63); the same reference in two reads of one run"""
    s = Stream()
    s.run([(0, 5, 10), (0, 5, 900)])
    s.run([(0, 1, 10), (0, 2, 20), (0, 2, 930), (0, 3, 40)])
    for n in (6, 7, 13, 14, 33, 63):
        mid = [(0, 1 + k % 14, 19 * k) for k in range(n - 2)]     # references 1 .. 14
        s.run([(0, 15, 1700)] + mid + [(0, 15, 5)])               # distance L - 1
        s.run(s.seg(2, first=n))
    s.run([(1, 4, 10), (1, 6, 20), (2, 4, 810), (2, 6, 30), (2, 4, 40)])
    s.shorts(20)
    return s


def case_repeat_at_every_distance():
    """per distance d = 1 .. 31 a segment of d + 1 records with a window to itself whose last record repeats the reference of
    its first, and no other record does: the walk has to take step d, whatever stretches it is made of"""
    s = Stream()
    for d in range(1, 32):
        s.run([(0, 15, 1700)] + [(0, k % 15, 23 * k) for k in range(d - 1)] + [(0, 15, 5)])
        s.run(s.seg(63, first=d))
    return s


def case_unique_on_the_last_lane():
    """a read whose one target is the window's last lane: runs of 30 + 30 records, then a run of three whose last record
    alone is mapped (lanes 60 .. 62), then a run that no longer fits; the same with a one-record run on lane 62"""
    s = Stream()
    s.run(s.seg(30, first=1)), s.run(s.seg(30, first=2))
    s.run([(0, None, 0), (0, None, 0), (0, 9, 350)])
    s.run(s.seg(12, first=3))
    s.shorts(11)                                                    # 86: a window starts here
    s.run(s.seg(62, first=4))
    s.run(s.seg(1, first=11))
    s.run(s.seg(40, first=5))
    s.shorts(25)
    return s


CASES = {f"length_{n}": case_length(n) for n in LENGTHS}
CASES.update({f.__name__[5:]: f for f in (case_run_ends_on_lane_63, case_slot_end, case_staged_end, case_long_run_past_the_stage,
                                          case_mates, case_unmapped, case_repeats, case_repeat_at_every_distance,
                                          case_unique_on_the_last_lane)})
CASES.update({f"size_{n}": (lambda n=n: (case_sizes(), n)) for n in SIZES})
FORMS = ("four", "packed", "marked", "any")


# ------------------------------------------------------------------------------------------- the order front.hip states
def expected_reads(rec: Records, bin_off: np.ndarray):
    """the target list read by read: [(reference | head bit, global bin | unique bit), ...] per read with a target"""
    key, flag, ref, pos = rec.read_key, rec.flag, rec.ref_id, rec.begin_pos
    reads, a, n = [], 0, len(rec)
    while a < n:
        b = a
        while b < n and key[b] == key[a]:
            b += 1
        for mate in (0, 1, 2):
            seen = {}
            for i in range(a, b):
                f = int(flag[i])
                m = 1 if f & 0x40 else (2 if f & 0x80 else 0)                  # src/slimm.hpp:205-208
                if m != mate or f & 4 or ref[i] < 0:                            # src/slimm.hpp:197
                    continue
                r = int(ref[i])
                if r not in seen:                                               # src/read_stat.hpp:125-131 (Q1)
                    seen[r] = int(bin_off[r]) + min(int(pos[i]) + READ_LEN // 2, int(REF_LEN[r])) // BIN
            if seen:
                reads.append([(r | (0x80000000 if k == 0 else 0), g | (0x80000000 if len(seen) == 1 else 0))
                              for k, (r, g) in enumerate(seen.items())])
        a = b
    return reads


def reads_of(ref, gbin):
    """the device's list cut at the head bits"""
    reads = []
    for r, g in zip(ref.tolist(), gbin.tolist()):
        if r >> 31:
            reads.append([])
        assert reads, "the list starts with a read's first target"
        reads[-1].append((r, g))
    return reads


_built = {}


def built(case):
    """the case's workload, the oracle's result and the expected reads: computed once, shared by the four forms"""
    if case not in _built:
        s = CASES[case]()
        s, n = s if isinstance(s, tuple) else (s, None)
        w = s.workload(case, n)
        assert 1 <= len(w.records) <= 4 * SLOT and N_REFS <= 16
        o = run_workload(w, use_qnames=False)
        assert not o.no_hits
        bin_off = np.concatenate([[0], np.cumsum((o.nbins.astype(np.int64) + 3) // 4 * 4)])
        _built[case] = (w, o, expected_reads(w.records, bin_off))
    return _built[case]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_front_windows(case, form):
    w, o, want = built(case)
    g = Slimm.for_workload(w, device=0, grouped=form != "any")
    if form == "packed":
        g.push_records_packed(w.records)
    elif form == "marked":
        g.push_records_marked(w.records)
    else:
        g.push_records(w.records)
    assert g.get_profiles() is not None
    got = reads_of(*g.read_targets())
    if form == "any":   # the grouping orders the reads by their identity, not by the file
        got, want = sorted(got), sorted(want)
    assert len(got) == len(want), f"{len(got)} reads with a target, not {len(want)}"
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"read {k}: targets {[(hex(r), hex(x)) for r, x in a]}, not {[(hex(r), hex(x)) for r, x in b]}"
    assert_matches_oracle(g, o)
    g.close()


def test_the_cases_hold_what_they_are_for():
    """the streams are what their names say (the positions the cases count on)"""
    s = case_slot_end()
    k = np.array(s.key)
    assert k[759] != k[760] and np.all(k[760:780] == k[760]) and k[780] != k[760]
    assert k[SLOT + 766] != k[SLOT + 767] and np.all(k[SLOT + 767:SLOT + 807] == k[SLOT + 767])
    s = case_staged_end()
    k = np.array(s.key)
    assert k[766] != k[767] and k[799] == k[767] and k[800] != k[767] and np.all(k[800:850] == k[800]) and k[850] != k[800]
    s = case_long_run_past_the_stage()
    k = np.array(s.key)
    assert k[759] != k[760] and np.all(k[760:860] == k[760]) and k[860] != k[760]
    s = case_run_ends_on_lane_63()
    k = np.array(s.key)
    assert k[63] == k[60] and k[64] != k[63]
    s = case_unique_on_the_last_lane()
    k = np.array(s.key)
    assert k[60] == k[62] != k[63] and s.ref[62] == 9 and k[86] != k[85] and k[86 + 62] != k[86 + 61] and k[86 + 63] != k[86 + 62]
    s = case_sizes()
    k = np.array(s.key)
    for n in (64, 768, 769, 833):
        assert k[n - 1] == k[n], f"N = {n} cuts a run"
    assert len(s) >= max(SIZES)
