"""The record filter of the `slimm` command on a real MI355X: the command WITH -q / --require-flags / --exclude-flags /
--min-aligned / --min-identity on the full BAM file against the command WITHOUT them on the file less its dropped records.
The profile, -ro and -co files must be byte for byte equal -- through the device decoders, with --host-decode, and with
--devices 0,0 --split-input, where the members' summed counts must be the one-device counts (a record at a cut is judged
once).  The file's log line must carry the counts of the Python restatement (tests/record_filter_ref.py)."""
import os
import subprocess

import pytest

from tests import record_filter_inputs as I
from tests import record_filter_ref as R
from tests.bam_io import write_sldb
from tests.test_record_filter_host import cli_args

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
OUTPUTS = ("_profile", "_raw", "_coverage", "_uniq_coverage", "_uniq_coverage2")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """full/sample.bam, pre/sample.bam (the records the restatement keeps under FILTERS["all"]), the database, the counts."""
    tmp = tmp_path_factory.mktemp("rf_cli")
    w, attrs, _lost = I.workload_and_attrs(grouped=True)
    bodies = I.bam_bodies(w, attrs)
    verdicts = [R.judge_bam(I.FILTERS["all"], b) for b in bodies]
    I.input_conditions(w, {"all": verdicts})
    keep = [not R.dropped(v) for v in verdicts]
    os.makedirs(tmp / "full")
    os.makedirs(tmp / "pre")
    I.bam_file(str(tmp / "full" / "sample.bam"), w, bodies, block=20_000)
    I.bam_file(str(tmp / "pre" / "sample.bam"), I.subset(w, keep), [b for b, k in zip(bodies, keep) if k], block=20_000)
    db = str(tmp / "db.sldb")
    write_sldb(db, w.taxonomy)
    return tmp, w, db, R.count(verdicts)


def run_slimm(tmp, w, db, which, tag, extra):
    out = str(tmp / tag) + "/"
    os.makedirs(out)
    args = ["-w", str(w.options.bin_width), "-o", out, "-ro", "-co", "-v"] + extra + [db, str(tmp / which / "sample.bam")]
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=dict(os.environ, SLIMM_TRACE="cli"))
    assert r.returncode == 0, r.stderr[-3000:]
    return {s: open(os.path.join(out, "sample" + s + ".tsv")).read() for s in OUTPUTS}, r.stderr


def filter_lines(err):
    return [ln.strip() for ln in err.split("\n") if ln.strip().startswith("record filter:")]


@pytest.fixture(scope="module")
def wanted(files):
    """The pre-filtered file without options, through the device decoders: run once."""
    tmp, w, db, _ = files
    got, err = run_slimm(tmp, w, db, "pre", "pre_out", [])
    assert not filter_lines(err) and got["_profile"].count("\n") > 1
    return got


@pytest.mark.parametrize("tag,extra", [("device", []), ("host", ["--host-decode"]), ("small_windows", ["--window-mb", "1", "--device-inflate", "2"])])
def test_options_on_the_full_file_equal_no_options_on_the_prefiltered_file(files, wanted, tag, extra):
    tmp, w, db, counts = files
    got, err = run_slimm(tmp, w, db, "full", "full_" + tag, cli_args(I.FILTERS["all"]) + extra)
    for s in OUTPUTS:
        assert got[s] == wanted[s], s
    assert filter_lines(err) == [R.stats_line(counts)]
    if tag == "host":   # (the same files without options through the host decoder too)
        pre, _ = run_slimm(tmp, w, db, "pre", "pre_host", ["--host-decode"])
        assert pre == wanted


def test_split_input_judges_a_record_at_a_cut_once(files, wanted):
    tmp, w, db, counts = files
    extra = ["--devices", "0,0", "--split-input", "--window-mb", "1"]
    got, err = run_slimm(tmp, w, db, "full", "full_split", cli_args(I.FILTERS["all"]) + extra)
    pre, pre_err = run_slimm(tmp, w, db, "pre", "pre_split", extra)
    assert "device decode on member 0" not in err   # (the members read their own ranges)
    assert got == pre and not filter_lines(pre_err)
    assert got["_profile"] == wanted["_profile"]
    assert filter_lines(err) == [R.stats_line(counts)]   # the members' sum = the one-device counts = the restatement's
    plain, plain_err = run_slimm(tmp, w, db, "full", "full_group", cli_args(I.FILTERS["all"]) + ["--devices", "0,0"])
    assert plain == got and filter_lines(plain_err) == [R.stats_line(counts)]
