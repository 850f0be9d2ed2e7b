"""A file in no particular order through a group on the device decoders (slimm_amd/csrc/deal_by_key.hip, group.hip): split by
byte range over the members (SlimmGroup.push_split on a group made with grouped=False: slimm_group_stitch_ranges joins the cuts,
then every member partitions its records by owner and takes its stretch of every member's), or pushed to member 0, whose records
slimm_group_get_profiles deals in the same way.  Every read ends up on one member, its records in the file's order; every
integer and the profile must be the oracle's.  (The inputs are small: the file also runs on the host emulator, SLIMM_EMU=1.)"""
import subprocess

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import SlimmGroup
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.workload import Records, Workload
from tests.bam_io import bam_record_bytes, sam_header, write_bam, write_sam
from tests.cases import holes_case, tiny_case
from tests.helpers import assert_matches_oracle, assert_profiles_match, force
from tests.sam_gz import bgzf, header_len
from tests.test_cli_gpu import CLI
from tests.test_gpu_bam_decode import _named
from tests.test_gpu_split_sam import split_and_check

pytestmark = pytest.mark.gpu

UNSORTED = "@HD\tVN:1.6\tSO:unsorted"
FORMS = ["bam", "sam", "bgzf_sam"]
CASES = {"tiny": tiny_case, "holes": holes_case,
         "config1": lambda: make_workload(CONFIGS["config1"], seed=43, n_records=4000, shuffled=True)}
_made = {}


def case(name):
    """(the named workload, the oracle's result): made once, never changed"""
    if name not in _made:
        w = _named(CASES[name]())
        _made[name] = (w, run_workload(w, use_qnames=True))
    return _made[name]


def file_of(tmp_path, w, form, tail_newline=True):
    """(the file's bytes or its path, the header skip its pushes take)"""
    if form == "bam":
        p = str(tmp_path / "x.bam")
        write_bam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, hd=UNSORTED, irregular_seed=5)
        text = sam_header(w.ref_names, w.ref_len, UNSORTED).encode()
        return p, 12 + len(text) + sum(8 + len(n.encode()) + 1 for n in w.ref_names)
    p = str(tmp_path / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, hd=UNSORTED)
    text = open(p, "rb").read()
    if not tail_newline:
        text = text[:-1]
    skip = header_len(text)
    return (text if form == "sam" else bgzf(text, seed=2, lo=100, hi=400)), skip


def held(g, members):
    return [g.member(i).records_held()[0] for i in range(members)]


def split_any_order(w, o, data, form, skip, members, window=0, bins=False):
    g = SlimmGroup(w, [0] * members, grouped=False)
    if bins:
        g.set_exchange("bins")
    offs, counts = g.push_split(data, form, skip=skip, window=window)
    after = held(g, members)
    assert sum(after) == len(w.records)
    assert g.get_profiles()
    s = g.member(0)
    assert_matches_oracle(s, o, bins=False)
    assert_profiles_match(s.write_abundance(), o.profile_tsv)
    if bins:   # (member 0 holds the global arrays)
        for k, want in enumerate((o.cov, o.uniq_cov, o.uniq_cov2)):
            assert np.array_equal(s.bins(k), want), k
    g.close()
    return offs, counts, after


@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_any_order_has_the_oracles_integers_and_profile(tmp_path, name, form, members):
    w, o = case(name)
    data, skip = file_of(tmp_path, w, form)
    offs, counts, after = split_any_order(w, o, data, form, skip, members)
    if name == "config1":
        assert all(b > a for a, b in zip(offs, offs[1:]))   # (every member has bytes of its own)
        assert min(after) > 0                                # ... and holds records after the stitch


@pytest.mark.parametrize("form", FORMS)
def test_split_any_order_in_small_windows(tmp_path, form):
    w, o = case("config1")
    data, skip = file_of(tmp_path, w, form)
    split_any_order(w, o, data, form, skip, 4, window=20_000)


@pytest.mark.parametrize("form", ["sam", "bgzf_sam"])
def test_split_any_order_last_line_without_newline(tmp_path, form):
    w, o = case("config1")
    data, skip = file_of(tmp_path, w, form, tail_newline=False)
    split_any_order(w, o, data, form, skip, 4)


@pytest.mark.parametrize("form", FORMS)
def test_split_any_order_more_members_than_lines(tmp_path, form):
    """Sixteen members for the tiny case: ranges that are all head and empty ranges send and receive empty stretches."""
    w, o = case("tiny")
    data, skip = file_of(tmp_path, w, form)
    split_any_order(w, o, data, form, skip, 16)


@pytest.mark.parametrize("form", FORMS + ["bam_bytes"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_any_order_through_member_0_is_dealt_on_the_device(tmp_path, name, form):
    """The file's windows pushed to member 0 and nothing through push_records*: get_profiles partitions member 0's records
    by owner and copies stretch i to member i."""
    w, o = case(name)
    members = 3
    g = SlimmGroup(w, [0] * members, grouped=False)
    m0 = g.member(0)
    if form == "bam_bytes":
        n = m0.push_bam_bytes(bam_record_bytes(w.records, read_len=w.avg_read_len, irregular_seed=5), window=50_000)
    else:
        data, skip = file_of(tmp_path, w, form)
        if form == "bam":
            n = m0.push_bgzf_blocks(open(data, "rb").read(), skip=skip)
        elif form == "sam":
            m0.set_reference_names(w.ref_names)
            n = m0.push_sam_bytes(data[skip:], window=30_000)
        else:
            m0.set_reference_names(w.ref_names)
            n = m0.push_bgzf_blocks(data, skip=skip, sam=True)
    assert n == len(w.records) and held(g, members) == [n, 0, 0]
    assert g.get_profiles()
    after = held(g, members)
    assert sum(after) == n
    if name == "config1":
        assert min(after) > 0
    assert_matches_oracle(g.member(0), o, bins=False)
    assert_profiles_match(g.member(0).write_abundance(), o.profile_tsv)
    g.close()


def two_records_apart():
    """config1 with 200 reads that each have two records on the SAME reference in DIFFERENT bins, one in the file's first
    quarter and one in its last: which of the two comes first in the file decides the read's bin (reference
    src/read_stat.hpp:116-135).  Also the workload with each such pair swapped."""
    w = make_workload(CONFIGS["config1"], seed=47, n_records=4000, shuffled=True)
    r = w.records
    n = len(r)
    first = np.nonzero((r.ref_id[:n // 4] >= 0) & ((r.flag[:n // 4] & 4) == 0))[0][:200]
    last = np.arange(n - 200, n)
    assert len(first) == 200
    key, flag, ref, pos = (np.array(a, copy=True) for a in (r.read_key, r.flag, r.ref_id, r.begin_pos))
    bw = w.options.bin_width
    key[last], flag[last], ref[last] = key[first], flag[first], ref[first]
    room = np.asarray(w.ref_len)[ref[first]].astype(np.int64)
    pos[last] = np.where(pos[first] + 4 * bw < room, pos[first] + 3 * bw, pos[first] - 3 * bw)
    assert (pos[last] >= 0).all()

    def made(order):
        rec = Records(key[order], flag[order], ref[order], pos[order], None)
        return _named(Workload(w.ref_names, w.ref_len, w.taxonomy, rec, w.avg_read_len, w.options, w.name, grouped=False))
    same = np.arange(n)
    swapped = same.copy()
    swapped[first], swapped[last] = last, first
    return made(same), made(swapped)


@pytest.mark.parametrize("form", FORMS)
def test_file_order_survives_the_deal(tmp_path, form):
    w, ws = two_records_apart()
    o, os_ = run_workload(w, use_qnames=True), run_workload(ws, use_qnames=True)
    assert not np.array_equal(o.cov, os_.cov)   # (the order of the two records matters: otherwise this shows nothing)
    data, skip = file_of(tmp_path, w, form)
    split_any_order(w, o, data, form, skip, 4, bins=True)


def host_keys(path):
    """the host reader's key of every record of the file (the command's --dump-records, no GPU)"""
    out = subprocess.run([CLI, "--dump-records", path], capture_output=True, text=True, check=True).stdout.splitlines()
    return np.array([int(ln.split("\t")[5]) for ln in out[1:] if ln and not ln.startswith("@\t")], dtype=np.uint64)


@pytest.mark.parametrize("members", [3, 4])
def test_the_device_deals_as_the_host_does(tmp_path, members):
    """The same file through the host's dealing (slimm_group_push_records_checked: key mod n on one thread) and through
    push_split: every member holds the same number of records."""
    w, o = case("config1")
    path, skip = file_of(tmp_path, w, "bam")
    key = host_keys(path)
    r = w.records
    assert len(key) == len(r)
    chk = ((key * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(32)).astype(np.uint32)
    g = SlimmGroup(w, [0] * members, grouped=False)
    g.push_records_checked(Records(key, r.flag, r.ref_id, r.begin_pos, None), chk, batch=700)
    by_host = held(g, members)
    g.close()
    assert by_host == np.bincount((key & np.uint64((1 << 62) - 1)) % np.uint64(members), minlength=members).tolist()
    _, _, by_device = split_any_order(w, o, path, "bam", skip, members)
    assert by_device == by_host


@pytest.mark.parametrize("form", FORMS)
def test_split_any_order_head_off_by_one_is_refused(tmp_path, monkeypatch, form):
    w, _ = case("config1")
    data, skip = file_of(tmp_path, w, form)
    g = SlimmGroup(w, [0, 0, 0], grouped=False)
    force(monkeypatch, split_shift_guess=1)
    with pytest.raises(capi.SlimmError) as e:
        g.push_split(data, form, skip=skip)
    assert e.value.code == capi.E_SPLIT
    g.close()


def test_a_grouped_group_still_stitches_as_before(tmp_path):
    w = _named(make_workload(CONFIGS["config1"], seed=41, n_records=4000))
    p = str(tmp_path / "g.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(p, "rb").read()
    split_and_check(w, text, "sam", header_len(text), 4)
