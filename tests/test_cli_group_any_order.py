"""`slimm --devices ...` on a file in no particular order, on a real MI355X: member 0's device decoders read the file and the
records are dealt to the members by key on the device; with --split-input every member reads its own byte range and the
stitch deals them (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE RANGE").  The five output files must be the ones one device
writes, byte for byte, and the profile the oracle's.  One context that meets the record cap reads the file again by byte range;
--host-decode keeps the host reader."""
import os
import re

import pytest

from oracle.binding import Oracle
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_bam, write_sam, write_sldb
from tests.cases import Q18_APART_EXPECTED, holes_case, q18_apart_case, tiny_case
from tests.helpers import assert_profiles_match
from tests.sam_gz import bgzf
from tests.test_cli_gpu import check_outputs, run_cli, with_names
from tests.test_cli_split_input import OUTPUTS, members_of

pytestmark = pytest.mark.gpu

UNSORTED = "@HD\tVN:1.6\tSO:unsorted"
FORMS = ["bam", "sam", "bgzf"]
INPUT = {"bam": "sample.bam", "sam": "sample.sam", "bgzf": "sample.sam.gz"}
STEM = {"bam": "sample", "sam": "sample", "bgzf": "sample.sam.gz"}   # (only .sam / .bam are taken off the name)
CASES = {"tiny": tiny_case, "holes": holes_case,
         "config1": lambda: make_workload(CONFIGS["config1"], seed=45, n_records=4000, shuffled=True)}


def write_input(tmp_path, w, form, hd=UNSORTED):
    db, inp = str(tmp_path / "db.sldb"), str(tmp_path / INPUT[form])
    if not os.path.exists(db):
        write_sldb(db, w.taxonomy)
        if form == "bam":
            write_bam(inp, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, hd=hd)
        else:
            sam = inp if form == "sam" else str(tmp_path / "text.sam")
            write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, hd=hd)
            if form == "bgzf":
                open(inp, "wb").write(bgzf(open(sam, "rb").read(), seed=7, lo=2_000, hi=9_000))
                os.remove(sam)   # (the command is given one file)
    return db, inp


def files_of(tmp_path, w, form, tag, extra, env=None, hd=UNSORTED):
    db, inp = write_input(tmp_path, w, form, hd)
    out = str(tmp_path / tag) + "/"
    os.makedirs(out)
    e = dict(os.environ, SLIMM_TRACE="cli")
    e.update(env or {})
    err = run_cli(["-w", str(w.options.bin_width), "-o", out, "-ro", "-co", "-v", "--window-mb", "1"] + extra + [db, inp], env=e)
    return {s: open(os.path.join(out, STEM[form] + s + ".tsv")).read() for s in OUTPUTS}, err


def dealt(err):
    return [tuple(int(x) for x in m) for m in re.findall(r"dealt by key: member (\d+) holds (\d+) records \((\d+) of its own\)", err)]


def group_matches_one_device(tmp_path, w, form, extra, env=None):
    one, err1 = files_of(tmp_path, w, form, "one", [])
    assert "dealt by key" not in err1
    got, err = files_of(tmp_path, w, form, "group", extra, env=env)
    assert got == one
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=False)
    assert_profiles_match(got["_profile"], o.profile_tsv)
    return err


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_group_reads_an_unsorted_file_through_member_0_and_deals_on_the_device(tmp_path, name, form):
    w = with_names(CASES[name]())
    err = group_matches_one_device(tmp_path, w, form, ["--devices", "0,0,0"])
    assert "device decode on member 0" in err, err[-3000:]
    d = dealt(err)
    assert [m[0] for m in d] == [0, 1, 2] and sum(m[1] for m in d) == len(w.records)
    assert d[0][2] == d[0][1] and d[1][2] == 0 and d[2][2] == 0   # (all of them were member 0's)
    if name == "config1":
        assert min(m[1] for m in d) > 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_input_on_an_unsorted_file(tmp_path, name, form):
    w = with_names(CASES[name]())
    err = group_matches_one_device(tmp_path, w, form, ["--devices", "0,0,0,0", "--split-input"])
    assert "split input:" not in err, err[-3000:]
    assert len(members_of(err)) == 4 and "device decode on member 0" not in err
    d = dealt(err)
    assert len(d) == 4 and sum(m[1] for m in d) == len(w.records)


@pytest.mark.parametrize("form", FORMS)
def test_split_input_head_off_by_one_falls_back_to_member_0(tmp_path, form):
    w = with_names(CASES["config1"]())
    err = group_matches_one_device(tmp_path, w, form, ["--devices", "0,0,0,0", "--split-input"], env={"SLIMM_FORCE": "split_shift_guess"})
    assert "split input:" in err and "reading the file through member 0" in err
    assert "device decode on member 0" in err and len(dealt(err)) == 4


def test_one_device_takes_more_unsorted_records_than_one_context(tmp_path):
    """SLIMM_FORCE record_cap: a context takes a third of the file's records; contexts of a group on the one device read a
    byte range each and deal the records by key."""
    w = with_names(CASES["config1"]())
    one, _ = files_of(tmp_path, w, "bam", "one", [])
    n = len(w.records.read_key)
    got, err = files_of(tmp_path, w, "bam", "capped", [], env={"SLIMM_FORCE": f"record_cap={n // 3}"})
    assert got == one
    assert "reading the file by byte range" in err and dealt(err)


def test_second_reading_of_a_q18_file_is_split_too(tmp_path):
    """A file grouped by QNAME whose shortened names stand apart from their namesakes is read again in any order: under
    --devices --split-input that reading goes by byte range as well."""
    w = q18_apart_case()
    got, err = files_of(tmp_path, w, "bam", "split", ["--devices", "0,0,0,0", "--split-input"], hd="@HD\tVN:1.6\tSO:unsorted\tGO:query")
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=True, want_cov=True)
    check_outputs(str(tmp_path / "split"), "sample", o)
    again = err.split("again as a file in no particular order", 1)
    assert len(again) == 2
    assert len(members_of(again[1])) == 4 and len(dealt(again[1])) == 4
    assert f"{Q18_APART_EXPECTED['matches']} matching reads" in err


def test_host_decode_keeps_the_host_reader(tmp_path):
    w = with_names(CASES["config1"]())
    err = group_matches_one_device(tmp_path, w, "bam", ["--devices", "0,0,0", "--host-decode"])
    assert "device decode on member 0" not in err and not dealt(err)
