"""The two forms of a target's reference word (slimm_amd/csrc/kernels.h: TargetRefs): 16 bits -- the reference in bits
0-14, "first target of its read" in bit 15 -- for a database of at most 32 768 references, 32 bits otherwise or with
SLIMM_FORCE ref16=0.  k_front writes the word at five places (the fast windows, the two passes of the staged long run,
the long run beyond the stage, and all of them again behind the grouping of record_order = ANY), k_filter_compact reads
it in full batches from one base and in a clamped partial batch, filter_span / k_filter_walk read it for the slots with
a read of 64 valid targets or more.

Every case runs in both forms and both must give the oracle's numbers; where the target list is known it is compared
too (slimm_get_read_targets gives the 32-bit form whatever the device holds).  The hand-built streams are those of
tests/test_gpu_front_windows.py and tests/test_gpu_filter_batches.py, imported; the databases of 32 768 and 32 769
references are short references at a small bin width, as the many-refs configuration of tests/test_gpu_scatter_rounds.py.

Inputs stay far below 300 K records: with SLIMM_EMU=1 (tests/native) the file runs on the CPU, where device memory is
filled with a poison pattern -- a reader that takes 4 bytes where 2 were written reads poison.
"""
import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from slimm_amd.synth import synth_taxonomy
from slimm_amd.workload import Options, Records, Workload
from tests import test_gpu_filter_batches as fb
from tests import test_gpu_front_windows as fw
from tests.helpers import assert_matches_oracle, force

pytestmark = pytest.mark.gpu

SLOT = 768
WIDTHS = ("ref16", "ref32")   # the form the library picks for a small database, and SLIMM_FORCE ref16=0


def set_width(monkeypatch, width, n_refs):
    """forces the 32-bit form where asked; returns the width the context must report"""
    if width == "ref32":
        force(monkeypatch, ref16=0)
    return 16 if width == "ref16" and n_refs <= 32768 else 32


# ------------------------------------------------------------------------------- databases of 32 768 and 32 769 references
BIG_LEN, BIG_BIN, BIG_READ = 250, 100, 100
LAST16 = 32767   # the largest reference of the 16-bit form: with the head flag its word is 0xffff


def boundary_stream(n_refs):
    """short runs all over the database, and the top references in every place a target can have: reference 32767 (and
    the database's last) as a read's first target, as a later one, as a read's only one, as mate 2's head behind mate 1,
    inside interleaved mates, and at the start, in the middle and at the end of a run of 70 records"""
    s = fw.Stream()
    top = n_refs - 1
    far = lambda k: (k * 7919 + 13) % n_refs   # noqa: E731
    for k in range(40):
        s.run([(0, far(3 * k + j), 10 + 7 * j) for j in range(1 + k % 4)])
    for r in sorted({LAST16, top}):
        s.run([(0, r, 10), (0, 5, 20)])                                    # first target of its read
        s.run([(0, 7, 10), (0, r, 30), (0, r - 1, 40), (0, r, 90)])         # a later one (and a repeat: Q1)
        s.run([(0, r, 50)])                                                # the only one: head and unique
        s.run([(1, 3, 10), (1, r, 20), (2, r, 30), (2, 9, 40)])             # mate 2's head
        s.run([(1, r, 10), (2, r - 1, 20), (1, 4, 30), (2, r, 40)])         # interleaved mates: the general path
        s.run([(0, r, 5)] + [(0, far(k), 3 * k) for k in range(33)] + [(0, r, 60)])   # 35 records: the hash path of a window
        s.run([(0, r, 5)] + [(0, r - 2 - k, 3 * k) for k in range(40)] + [(0, r - 1, 9)] + [(0, r - 2 - k, 2 * k) for k in range(28)])
        s.run([(0, 11, 5)] + [(0, r - 50 - k, 3 * k) for k in range(68)] + [(0, r, 9)])        # 70 records, the top one last
        s.run([(1, r - k, 3 * k) for k in range(40)] + [(2, r - k, 2 * k) for k in range(39, -1, -1)])   # 80: two mates
    for k in range(40):
        s.run([(0, far(5 * k + j + 1000), 10 + 7 * j) for j in range(1 + k % 3)])
    return s


_boundary = {}


def boundary(n_refs):
    """the workload, the oracle's result: once per database, shared by the two forms"""
    if n_refs not in _boundary:
        s = boundary_stream(n_refs)
        rec = Records(np.array(s.key, dtype=np.uint64), np.array(s.flag, dtype=np.uint16),
                      np.array(s.ref, dtype=np.int32), np.array(s.pos, dtype=np.int32))
        tax = synth_taxonomy(n_refs)
        w = Workload([a + ".1" for a in tax.accessions], np.full(n_refs, BIG_LEN, dtype=np.uint32), tax, rec,
                     avg_read_len=BIG_READ, options=Options(bin_width=BIG_BIN), name=f"refs-{n_refs}")
        _boundary[n_refs] = (w, run_workload(w, use_qnames=False))
    return _boundary[n_refs]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n_refs", [32768, 32769])
def test_database_at_the_boundary(monkeypatch, n_refs, width):
    bits = set_width(monkeypatch, width, n_refs)
    w, o = boundary(n_refs)
    assert len(w.records) < 2 * SLOT and int(w.records.ref_id.max()) == n_refs - 1
    g = Slimm.for_workload(w, device=0)
    assert g.target_ref_bits() == bits, "32 768 references take the 16-bit form unless forced, 32 769 never do"
    g.push_records(w.records)
    assert g.get_profiles() is not None and not o.no_hits
    ref, gbin = g.read_targets()
    for r in {LAST16, n_refs - 1}:
        assert (ref == (r | 0x80000000)).any(), f"reference {r} as a read's first target"
        assert (ref == r).any(), f"reference {r} as a later target"
        assert ((ref == (r | 0x80000000)) & (gbin >> 31 != 0)).any(), f"reference {r} as a read's only target"
    assert int((ref & 0x7fffffff).max()) == n_refs - 1
    assert_matches_oracle(g, o)
    g.close()


# --------------------------------------------------------------------------------------- every store site of the front end
# fast windows below and above the hash-table threshold, runs of 64 records and more inside the staged stretch and beyond
# it, runs across slots, interleaved mates (the general path), unmapped records
FRONT_CASES = ("length_13", "length_33", "length_64", "length_65", "slot_end", "staged_end", "long_run_past_the_stage", "mates",
               "unmapped", "size_833")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("form", ["four", "marked"])
@pytest.mark.parametrize("case", FRONT_CASES)
def test_store_sites(monkeypatch, case, form, width):
    bits = set_width(monkeypatch, width, fw.N_REFS)
    w, o, want = fw.built(case)
    g = Slimm.for_workload(w, device=0)
    assert g.target_ref_bits() == bits
    if form == "marked":
        g.push_records_marked(w.records)
    else:
        g.push_records(w.records)
    assert g.get_profiles() is not None
    got = fw.reads_of(*g.read_targets())
    assert got == want
    assert_matches_oracle(g, o)
    g.close()


_interleaved = {}


def interleaved():
    """the `mates` stream with its records dealt out of order -- no two records of a qName run need be neighbours: what
    record_order = ANY is for"""
    if not _interleaved:
        w, _, _ = fw.built("mates")
        r = w.records
        perm = np.random.Generator(np.random.PCG64(16)).permutation(len(r))
        rec = Records(r.read_key[perm], r.flag[perm], r.ref_id[perm], r.begin_pos[perm])
        assert (rec.read_key[1:] == rec.read_key[:-1]).mean() < 0.2
        w2 = Workload(w.ref_names, w.ref_len, w.taxonomy, rec, w.avg_read_len, w.options, "mates-interleaved")
        _interleaved["w"] = (w2, run_workload(w2, use_qnames=False))
    return _interleaved["w"]


@pytest.mark.parametrize("width", WIDTHS)
def test_sorted_front_end(monkeypatch, width):
    bits = set_width(monkeypatch, width, fw.N_REFS)
    w, o = interleaved()
    g = Slimm.for_workload(w, device=0, grouped=False)
    assert g.target_ref_bits() == bits
    g.push_records(w.records)
    assert g.get_profiles() is not None and not o.no_hits
    assert_matches_oracle(g, o)
    g.close()


# ------------------------------------------------------------------ a slot whose targets begin at an odd index of the array
def odd_start_stream():
    """Three unmapped records in front, and a run over records 765 .. 768: the second slot's first run starts at record
    769, so its targets lie from index 769 on -- a run of 16-bit words that begins off a 4-byte boundary, more than 300
    targets long (a full batch of the filter from an odd base, and a partial one)."""
    s = fw.Stream()
    s.run([(0, None, 0)] * 3)
    s.upto(765)
    s.run(s.seg(4, first=3))            # 765 .. 768
    for k in range(150):                # 769 .. 1068: every record a target
        s.run(s.seg(2, first=k))
    s.shorts(41)
    return s


_odd = {}


@pytest.mark.parametrize("width", WIDTHS)
def test_slot_starting_at_an_odd_target(monkeypatch, width):
    bits = set_width(monkeypatch, width, fw.N_REFS)
    if not _odd:
        s = odd_start_stream()
        k = np.array(s.key)
        assert k[764] != k[765] and k[768] == k[765] and k[769] != k[768] and k[770] == k[769] and k[771] != k[770]
        w = s.workload("odd-start")
        o = run_workload(w, use_qnames=False)
        bin_off = np.concatenate([[0], np.cumsum((o.nbins.astype(np.int64) + 3) // 4 * 4)])
        _odd["w"] = (w, o, fw.expected_reads(w.records, bin_off))
    w, o, want = _odd["w"]
    g = Slimm.for_workload(w, device=0)
    assert g.target_ref_bits() == bits
    g.push_records(w.records)
    assert g.get_profiles() is not None and not o.no_hits
    assert fw.reads_of(*g.read_targets()) == want
    assert_matches_oracle(g, o)
    g.close()


# ---------------------------------------------------------------------------------------------- the filter's three readers
def readers_stream():
    s = fb.Stream(16)
    s.preamble()
    s.slot(s.short_reads(300))                                                     # a full batch and a partial one
    s.slot(s.short_reads(256))                                                     # exactly one full batch
    s.slot(s.short_reads(37))                                                      # a partial batch alone
    s.slot(s.short_reads(100) + [fb.valid_run(66, 3)] + s.short_reads(150))        # 66 valid targets: k_filter_walk's slot
    s.slot(fb.singles(200) + [fb.valid_run(64, 1)] + s.short_reads(247))           # ... and across the first batch's end
    s.ordinary()
    return s


_readers = {}


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("rows", ["rows16", "rows32"])
def test_filter_readers(monkeypatch, rows, width):
    bits = set_width(monkeypatch, width, fb.N_REFS)
    if rows == "rows32":
        force(monkeypatch, wide_rows=1)
    if not _readers:
        s = readers_stream()
        w = s.workload("filter-readers")
        assert len(w.records) % SLOT == 0
        _readers["w"] = (s, w, run_workload(w, use_qnames=False))
    s, w, o = _readers["w"]
    assert o.valid[fb.GOOD].all() and not o.valid[fb.BAD].any(), "good references are valid, bad ones are not"
    g = Slimm.for_workload(w, device=0)
    assert g.target_ref_bits() == bits
    g.push_records(w.records)
    assert g.get_profiles() is not None and not o.no_hits
    ref, _ = g.read_targets()
    assert np.array_equal(ref & 0x7fffffff, np.array(s.targets, dtype=np.uint32))
    assert np.array_equal((ref >> 31) != 0, np.array(s.heads))
    assert_matches_oracle(g, o)
    g.close()
