"""The record filter in the device decoders (k_bam_decode / k_sam_decode with kFilter: bam_decode.hip, sam_decode.hip;
slimm_set_record_filter) on a real MI355X, at library level: a context WITH the filter that is pushed the full file must
equal a context WITHOUT one that is pushed the file less its dropped records -- in read targets, taxon counts at both
stages, the integer statistics and the profile text -- and slimm_get_record_filter_stats must equal the count of the Python
restatement (tests/record_filter_ref.py) exactly.  The same 4 000 records over 8 references go in as BAM bytes, BGZF blocks,
SAM text and gzip-compressed SAM, through the run-marked instantiation (SLIMM_ORDER_GROUPED) and the four-array one
(SLIMM_ORDER_ANY), in windows as small as tests/test_gpu_bam_decode.py and tests/test_gpu_stream_sam.py force them, so that
records with 40-operation CIGARs and long tag areas straddle pieces and windows."""
import ctypes as C
import random

import numpy as np
import pytest

from slimm_amd import capi
from slimm_amd.profiler import Slimm, SlimmGroup
from tests import record_filter_inputs as I
from tests import record_filter_ref as R
from tests import sam_deflate as D
from tests.sam_gz import header_len

pytestmark = pytest.mark.gpu

FORMS = ["bam", "bgzf", "sam", "gzip"]
GZIP_FORCE = "gzip_chunk=2048,gzip_round=1"   # (tests/test_gpu_stream_sam.py: rounds as small as the pushes)

_cases, _wanted = {}, {}


def case(tmp_path, grouped):
    """The records, their SAM lines and BAM records, and every filter's verdicts by the restatement: made once per order."""
    if grouped not in _cases:
        w, attrs, _lost = I.workload_and_attrs(grouped=grouped)
        lines, bodies = I.sam_lines(w, attrs, tmp_path), I.bam_bodies(w, attrs)
        verdicts = {name: [R.judge_bam(f, b) for b in bodies] for name, f in I.FILTERS.items()}
        assert verdicts["all"] == [R.judge_sam(I.FILTERS["all"], ln) for ln in lines]
        I.input_conditions(w, verdicts)
        _cases[grouped] = (w, lines, bodies, verdicts)
    return _cases[grouped]


def set_filter(s, f):
    s.set_record_filter(min_mapq=f["min_mapq"], require_flags=f["require_flags"], exclude_flags=f["exclude_flags"],
                        min_aligned=f["min_aligned"], min_identity=f["min_identity_permille"] / 1000.0)


def cuts_of(n, seed, lo=1_500, hi=6_000):
    rng, p, out = random.Random(seed), 0, []
    while True:
        p += rng.randint(lo, hi)
        if p >= n:
            return out
        out.append(p)


def push(s, form, w, lines, bodies, small):
    if form == "bam":
        return s.push_bam_bytes(I.bam_bytes(bodies), window=16_411 if small else 0)
    if form == "bgzf":
        return s.push_bgzf_blocks(I.bgzf_of(I.bam_bytes(bodies), seed=5, lo=300, hi=9_000), skip=0, window=8_000 if small else 0)
    s.set_reference_names(w.ref_names)
    text = I.sam_file_text(w, lines, tail_newline=form == "gzip")   # (plain text: the last line, an NM field, ends the file)
    skip = header_len(text)
    if form == "sam":
        return s.push_sam_bytes(text[skip:], window=8_209 if small else 0)
    blob = D.copy_of(text, "mem1")
    return s.push_gzip_sam_bytes(blob, skip=skip, cuts=cuts_of(len(blob), 3))


def results(s, grouped):
    """What is compared.  A grouped file's read targets stand in file order: compared as they are.  In any order the reads
    stand in the order the grouping passes leave them in, which slimm_group_plan chooses by the NUMBER of records -- and the
    pre-filtered file has fewer: there the reads (a read starts where the reference word's top bit is set) are compared as a
    sorted list of reads."""
    text = s.get_profiles()
    st = {k: v for k, v in s.stats().items() if isinstance(v, (int, np.integer)) and k != "n_records"}
    ref, gbin = (np.asarray(a).tolist() for a in s.read_targets())
    targets = list(zip(ref, gbin))
    if not grouped:
        starts = [i for i, r in enumerate(ref) if r >> 31] + [len(ref)]
        assert not ref or starts[0] == 0
        targets = sorted(tuple(targets[a:b]) for a, b in zip(starts, starts[1:]))
    return dict(targets=targets, taxa0=s.taxon_counts(0), taxa1=s.taxon_counts(1), stats=st, profile=text)


def wanted(tmp_path, grouped, name):
    """No filter, the file less the records the restatement drops (as BAM bytes in one window): computed once, shared."""
    if (grouped, name) not in _wanted:
        w, lines, bodies, verdicts = case(tmp_path, grouped)
        keep = [not R.dropped(v) for v in verdicts[name]]
        wk = I.subset(w, keep)
        s = Slimm.for_workload(wk, device=0, grouped=grouped)
        n = push(s, "bam", wk, None, [b for b, k in zip(bodies, keep) if k], small=False)
        assert n == sum(keep) < len(keep)
        out = results(s, grouped)
        assert s.record_filter_stats() == dict.fromkeys(R.STATS, 0)
        s.close()
        assert out["stats"]["hits_count"] > 0 and out["profile"]
        _wanted[(grouped, name)] = out
    return _wanted[(grouped, name)]


def check(tmp_path, monkeypatch, form, grouped, name):
    w, lines, bodies, verdicts = case(tmp_path, grouped)
    want = wanted(tmp_path, grouped, name)
    if form == "gzip":
        monkeypatch.setenv("SLIMM_FORCE", GZIP_FORCE)
    s = Slimm.for_workload(w, device=0, grouped=grouped)
    set_filter(s, I.FILTERS[name])
    assert push(s, form, w, lines, bodies, small=True) == len(w.records)
    assert s.record_filter_stats() == R.count(verdicts[name])
    got = results(s, grouped)
    for k in want:
        assert got[k] == want[k], k
    assert s.record_filter_stats() == R.count(verdicts[name])   # (analysing changes nothing)
    s.reset()
    assert s.record_filter_stats() == dict.fromkeys(R.STATS, 0)   # per file
    s.close()


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "any_order"])
@pytest.mark.parametrize("form", FORMS)
def test_filtered_file_equals_the_prefiltered_file(tmp_path, monkeypatch, form, grouped):
    check(tmp_path, monkeypatch, form, grouped, "all")


@pytest.mark.parametrize("form,grouped", [("bam", True), ("sam", False)], ids=["bam-grouped", "sam-any_order"])
@pytest.mark.parametrize("name", [n for n in I.FILTERS if n != "all"])
def test_each_criterion_alone(tmp_path, monkeypatch, name, form, grouped):
    check(tmp_path, monkeypatch, form, grouped, name)


def test_no_filter_and_a_filter_set_back_to_off_change_nothing(tmp_path):
    w, lines, bodies, _ = case(tmp_path, True)
    s = Slimm.for_workload(w, device=0, grouped=True)
    assert push(s, "bam", w, lines, bodies, small=True) == len(w.records)
    plain = results(s, True)
    s.reset()
    set_filter(s, I.FILTERS["all"])
    s.L.slimm_set_record_filter(s.ctx, None)   # NULL: off
    assert push(s, "bam", w, lines, bodies, small=True) == len(w.records)
    assert results(s, True) == plain and s.record_filter_stats() == dict.fromkeys(R.STATS, 0)
    s.close()


def test_the_filter_is_configuration(tmp_path):
    """Refused values; set before the file's first push, not after; it survives slimm_reset, the stats do not."""
    w, lines, bodies, verdicts = case(tmp_path, True)
    s = Slimm.for_workload(w, device=0, grouped=True)
    for bad in (dict(min_identity_permille=1001), dict(require_flags=0x10000), dict(exclude_flags=0x10000), dict(reserved=(0, 1, 0))):
        f = capi.RecordFilter(**bad)
        assert s.L.slimm_set_record_filter(s.ctx, C.byref(f)) == capi.E_INVALID, bad
        assert s.L.slimm_last_error(s.ctx)
    set_filter(s, I.FILTERS["mapq"])
    data = I.bam_bytes(bodies)
    got = C.c_uint64()
    half = np.frombuffer(data[:50_000], dtype=np.uint8).copy()
    assert s.L.slimm_push_bam_bytes(s.ctx, half.ctypes.data_as(C.c_void_p), half.size, 0, C.byref(got)) == capi.OK
    f = capi.RecordFilter(min_mapq=20)
    assert s.L.slimm_set_record_filter(s.ctx, C.byref(f)) == capi.E_INVALID
    assert b"before" in s.L.slimm_last_error(s.ctx)
    s.reset()
    assert s.push_bam_bytes(data, window=16_411) == len(w.records)       # (still -q 10: not 20, not off)
    assert s.record_filter_stats() == R.count(verdicts["mapq"])
    s.close()


def test_a_group_filters_every_range_once(tmp_path):
    """One BAM file split by byte range over three members on one device: every member judges the records of its own range --
    the record across a cut by the member on its left --, member 0 answers with the sum, and the group's profile is the
    pre-filtered file's."""
    w, lines, bodies, verdicts = case(tmp_path, True)
    want = wanted(tmp_path, True, "all")
    path = str(tmp_path / "split.bam")
    I.bam_file(path, w, bodies, block=6_000)
    g = SlimmGroup(w, [0, 0, 0], grouped=True)
    f = I.FILTERS["all"]
    g.set_record_filter(min_mapq=f["min_mapq"], require_flags=f["require_flags"], exclude_flags=f["exclude_flags"],
                        min_aligned=f["min_aligned"], min_identity=f["min_identity_permille"] / 1000.0)
    skip = len(I.bam_header_bytes(w.ref_names, w.ref_len))
    _offs, counts = g.push_split(path, "bam", skip=skip, window=20_000)
    assert all(counts)
    m0 = g.member(0)
    assert m0.record_filter_stats() == R.count(verdicts["all"])
    per_member = [g.member(i).record_filter_stats()["judged"] for i in (1, 2)]
    assert all(per_member) and sum(per_member) < m0.record_filter_stats()["judged"]
    assert g.get_profiles()
    assert m0.taxon_counts(1) == want["taxa1"] and m0.taxon_counts(0) == want["taxa0"]
    st = m0.stats()
    assert {k: st[k] for k in ("hits_count", "matches_count", "uniq_matches_count")} == {k: want["stats"][k] for k in ("hits_count", "matches_count", "uniq_matches_count")}
    g.close()
