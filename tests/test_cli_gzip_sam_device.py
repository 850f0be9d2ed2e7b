"""The `slimm` command on gzip copies of a SAM file, on a real MI355X: a regular gzip file's bytes go to the device
(slimm_push_gzip_sam_bytes) and every output file is the plain file's and the oracle's; --host-decode keeps the host reader.
SLIMM_TRACE=cli says which of the two read the file."""
import os
import subprocess

import pytest

from oracle.binding import Oracle
from slimm_amd.synth import CONFIGS, make_workload
from tests import sam_deflate as D
from tests.bam_io import write_sam, write_sldb
from tests.cases import q18_apart_case, tiny_case
from tests.test_cli_gpu import check_outputs, with_names
from tests.test_gpu_compressed_sam import CLI, outputs

pytestmark = pytest.mark.gpu

MODES = {
    "device": [],
    "host_decode": ["--host-decode"],
    "any_order": ["--any-order"],
    "devices": ["--devices", "0,0"],
    "window1": ["--window-mb", "1"],
}
TRACE_LINE = "gzip SAM on the device:"


def run_cli(args, force=None):
    env = dict(os.environ, SLIMM_TRACE="cli")
    if force:
        env["SLIMM_FORCE"] = force
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def cli_case(tmp_path, w, modes, kinds=("default", "mem1", "members"), tail_newline=True, force=None):
    w = with_names(w)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(sam, "rb").read()
    if not tail_newline:
        open(sam, "wb").write(text[:-1])
        text = text[:-1]
    copies = {kind: D.copy_of(text, kind) for kind in kinds}
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=True, want_cov=True)
    for mode in modes:
        base = ["-w", str(w.options.bin_width), "-ro", "-co"] + MODES[mode]
        plain_dir = str(tmp_path / f"plain_{mode}") + "/"
        os.makedirs(plain_dir)
        run_cli(base + ["-o", plain_dir, db, sam])
        want = outputs(plain_dir, "x")
        check_outputs(plain_dir, "x", o)
        for kind, blob in copies.items():
            d = str(tmp_path / f"{kind}_{mode}")
            os.makedirs(d)
            inp = os.path.join(d, "x.sam.gz")
            open(inp, "wb").write(blob)
            err = run_cli(base + [db, inp], force=force)   # (outputs next to the input: x.sam.gz keeps its whole name)
            assert outputs(d, "x.sam.gz") == want, (kind, mode)
            assert (TRACE_LINE in err) == (mode != "host_decode"), (kind, mode, err[-1500:])
            if mode != "host_decode":
                line = [ln for ln in err.split("\n") if TRACE_LINE in ln][0]
                assert f"{4 if kind == 'members' else 1} members" in line and f"{len(text)} bytes of text" in line, line


@pytest.mark.parametrize("case", ["tiny", "q18_apart", "config1"])
def test_cli_gzip_sam_writes_the_files_of_the_plain_sam(tmp_path, case):
    w = {"tiny": tiny_case, "q18_apart": q18_apart_case, "config1": lambda: make_workload(CONFIGS["config1"], seed=41)}[case]()
    cli_case(tmp_path, w, sorted(MODES), force="gzip_chunk=4096")


@pytest.mark.parametrize("tail_newline", [True, False])
def test_cli_gzip_sam_lines_straddle_chunks_rounds_and_windows(tmp_path, tail_newline):
    """200 000 records at memLevel 1 read in 1 MB windows and decoded every 300 kB of compressed bytes, in chunks of 16 kB:
    lines lie across chunks, rounds and windows, and the last line has its newline or not."""
    w = make_workload(CONFIGS["config2"], seed=45, n_records=200_000)
    cli_case(tmp_path, w, ["window1", "any_order"], kinds=("mem1",), tail_newline=tail_newline, force="gzip_chunk=16384,gzip_round=300000")


def test_cli_2m_record_gzip_sam_has_the_profile_of_the_plain_sam(tmp_path):
    w = with_names(make_workload(CONFIGS["config3"], seed=47, n_records=2_000_000))
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=100)
    d = str(tmp_path / "gz")
    os.makedirs(d)
    inp = os.path.join(d, "x.sam.gz")
    open(inp, "wb").write(D.member(open(sam, "rb").read()))   # (what `gzip x.sam` writes: level 6, one member)
    run_cli(["-w", "1000", "-o", str(tmp_path) + "/", db, sam])
    err = run_cli(["-w", "1000", db, inp])
    assert TRACE_LINE in err
    assert open(os.path.join(d, "x.sam.gz_profile.tsv"), "rb").read() == open(str(tmp_path / "x_profile.tsv"), "rb").read()
