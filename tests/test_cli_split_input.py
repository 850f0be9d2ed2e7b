"""`slimm --devices ... --split-input` on a real MI355X: every member of the group reads, inflates and decodes its own byte
range of a name-grouped BAM file and the cuts are stitched on the device (include/slimm_hip.h, "ONE BAM FILE SPLIT BY BYTE
RANGE").  The files must be the ones one device writes; a wrong guess must fall back to member 0; one device must take a
file of more records than one context holds."""
import os
import random
import re

import numpy as np
import pytest

from oracle.binding import Oracle
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.workload import Records, Workload
from tests.bam_io import write_bam, write_sldb
from tests.cases import Q18_APART_EXPECTED, holes_case, q18_apart_case, records_from_sam, tiny_case
from tests.helpers import assert_profiles_match
from tests.test_cli_gpu import check_outputs, run_cli, with_names

pytestmark = pytest.mark.gpu

OUTPUTS = ("_profile", "_raw", "_coverage", "_uniq_coverage", "_uniq_coverage2")


def config1():
    return make_workload(CONFIGS["config1"], seed=41)


def one_run(w: Workload, lo: int, hi: int) -> Workload:
    """records [lo, hi) become alignments of ONE read (the name of record lo)"""
    r = w.records
    key = np.array(r.read_key, copy=True)
    key[lo:hi] = key[lo]
    return with_names(Workload(w.ref_names, w.ref_len, w.taxonomy, Records(key, r.flag, r.ref_id, r.begin_pos, None, r.file_flag),
                               w.avg_read_len, w.options, w.name))


def files_of(tmp_path, w, tag, extra, env=None, bam_kw=None):
    db = str(tmp_path / "db.sldb")
    inp = str(tmp_path / "sample.bam")
    if not os.path.exists(db):
        write_sldb(db, w.taxonomy)
        write_bam(inp, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, **(bam_kw or {}))
    out = str(tmp_path / tag) + "/"
    os.makedirs(out)
    e = dict(os.environ, SLIMM_TRACE="cli")
    e.update(env or {})
    err = run_cli(["-w", str(w.options.bin_width), "-o", out, "-ro", "-co", "-v"] + extra + [db, inp], env=e)
    return {s: open(os.path.join(out, "sample" + s + ".tsv")).read() for s in OUTPUTS}, err


def split_matches_one_device(tmp_path, w, devices, env=None, bam_kw=None, oracle=True, fallback=False):
    one, _ = files_of(tmp_path, w, "one", [], bam_kw=bam_kw)
    got, err = files_of(tmp_path, w, "split", ["--devices", devices, "--split-input", "--window-mb", "1"], env=env, bam_kw=bam_kw)
    assert got == one
    if oracle:  # (a workload built here has no oracle of its own to trust more than the single-device run)
        o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=False)
        assert_profiles_match(got["_profile"], o.profile_tsv)
    assert ("device decode on member 0" in err) == fallback   # (today's path: member 0 reads the whole file)
    return err


def members_of(err):
    return [tuple(int(x) for x in m) for m in re.findall(r"split member (\d+): bytes \[(\d+), (\d+)\) of (\d+), (\d+) records", err)]


@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
@pytest.mark.parametrize("mk", [tiny_case, holes_case, config1], ids=["tiny", "holes", "config1"])
def test_split_input_writes_the_single_device_files(tmp_path, mk, devices):
    err = split_matches_one_device(tmp_path, with_names(mk()), devices)
    assert "split input:" not in err, err[-2000:]
    assert len(members_of(err)) == devices.count("0")


@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0", "0,0,0,0,0,0,0,0"])
def test_split_input_run_of_10000_records_across_a_cut(tmp_path, devices):
    w = config1()
    n = len(w.records.read_key)
    err = split_matches_one_device(tmp_path, one_run(w, n // 2 - 5000, n // 2 + 5000), devices, oracle=False)
    assert "split input:" not in err
    handed = [int(x) for x in re.findall(r"handed (\d+) records left", err)]
    assert max(handed) > 1000   # (the run's part behind a cut went to the member that holds its start)


def test_split_input_run_over_a_whole_middle_member(tmp_path):
    w = config1()
    n = len(w.records.read_key)
    err = split_matches_one_device(tmp_path, one_run(w, n // 8, 7 * n // 8), "0,0,0,0", oracle=False)
    assert "split input:" not in err
    assert re.search(r"member [12] handed \d+ records left to member 0, keeps 0", err), err[-3000:]


def test_split_input_cuts_inside_records_and_irregular_lengths(tmp_path):
    # (the sampled read length follows the irregular sequences: the single-device run is the yardstick here)
    err = split_matches_one_device(tmp_path, with_names(config1()), "0,0,0,0,0,0", bam_kw={"irregular_seed": 7}, oracle=False)
    assert "split input:" not in err
    heads = [int(x) for x in re.findall(r"cut in front of member \d+: (\d+) head bytes", err)]
    assert heads and max(heads) > 0   # (a range whose first block begins inside a record)


def test_split_input_members_without_a_record_start(tmp_path):
    # one record of 400 000 bases (~600 KB over ten BGZF blocks of a few hundred compressed bytes each) among the tiny
    # case's: ranges that lie inside it; then the tiny case alone, one block for eight members: empty ranges
    os.makedirs(tmp_path / "long")
    err = split_matches_one_device(tmp_path / "long", with_names(tiny_case()), "0,0,0,0,0,0,0,0", bam_kw={"l_seq_of": {30: 400_000}},
                                   oracle=False)
    assert "split input:" not in err
    assert any(m[4] == 0 and m[2] > m[1] for m in members_of(err)), err[-3000:]
    os.makedirs(tmp_path / "tiny")
    err = split_matches_one_device(tmp_path / "tiny", with_names(tiny_case()), "0,0,0,0,0,0,0,0")
    assert "split input:" not in err
    assert any(m[4] == 0 for m in members_of(err))


def test_split_input_every_member_reads_its_share(tmp_path):
    w = with_names(make_workload(CONFIGS["config1"], seed=41, n_records=200_000))
    err = split_matches_one_device(tmp_path, w, "0,0,0,0", oracle=False)
    ms = members_of(err)
    assert len(ms) == 4
    total = ms[0][3]
    for i, lo, hi, _, _ in ms:
        assert 0.5 * total / 4 <= hi - lo <= 1.5 * total / 4, ms


def test_split_input_wrong_guess_falls_back_to_member_0(tmp_path):
    err = split_matches_one_device(tmp_path, with_names(config1()), "0,0,0", env={"SLIMM_FORCE": "split_shift_guess"}, fallback=True)
    assert "split input:" in err and "reading the file through member 0" in err


def test_one_device_takes_more_records_than_one_context(tmp_path):
    """SLIMM_FORCE record_cap: a context takes a third of the file's records.  Without the split the command stops with
    the 2^31 error; with it, contexts of a group on the one device read a byte range each."""
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, "one", [])
    n = len(w.records.read_key)
    got, err = files_of(tmp_path, w, "capped", ["--window-mb", "1"], env={"SLIMM_FORCE": f"record_cap={n // 3}"})
    assert got == one
    assert "reading the file by byte range" in err


def test_split_input_q18_runs_apart_regroup_like_one_device(tmp_path):
    w = q18_apart_case()
    got, err = files_of(tmp_path, w, "split", ["--devices", "0,0,0,0", "--split-input"])
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=True, want_cov=True)
    check_outputs(str(tmp_path / "split"), "sample", o)
    assert "again as a file in no particular order" in err
    assert f"{Q18_APART_EXPECTED['matches']} matching reads" in err


def test_split_input_q18_pairs_across_cuts(tmp_path):
    """Every read is an unflagged `p.1` followed by `p` with the first-mate flag: one run each (Q18), no regroup -- also
    where a cut lies between the two records (the join moves the correction of the counts to the member on the right)."""
    t = tiny_case()
    rng = random.Random(3)
    rows = []
    for i in range(6000):
        rows.append((f"p{i}.1", 0, rng.choice(t.ref_names[:4]), rng.randint(1, 800)))
        rows.append((f"p{i}", 0x41, rng.choice(t.ref_names[:4]), rng.randint(1, 800)))
    w = Workload(t.ref_names, t.ref_len, t.taxonomy, records_from_sam(rows, t.ref_names), avg_read_len=50, options=t.options,
                 name="q18-pairs")
    one, err1 = files_of(tmp_path, w, "one", [])
    got, err = files_of(tmp_path, w, "split", ["--devices", "0,0,0,0,0,0,0,0", "--split-input"])
    assert got == one
    assert "no particular order" not in err and "no particular order" not in err1
    assert "split input:" not in err
