"""The `slimm` command on xz copies of a SAM file, on a real MI355X: a regular xz file of enough blocks goes to the device
(slimm_push_xz_sam_bytes) and every output file is the plain file's; --host-decode keeps the host reader; a group reads the
file through member 0, with --split-input too; a file of few blocks (by its index) is read on the host unless SLIMM_FORCE
xz_device_blocks says otherwise.  SLIMM_TRACE=cli says which of the two read the file.  The inputs: the committed files of
tests/golden/xz and containers written in Python (tests/sam_xz.py)."""
import os
import subprocess

import pytest

from tests import sam_xz as X
from tests.bam_io import write_sldb
from tests.test_gpu_compressed_sam import CLI, outputs

pytestmark = pytest.mark.gpu

MODES = {
    "device": [],
    "host_decode": ["--host-decode"],
    "any_order": ["--any-order"],
    "devices": ["--devices", "0,0"],
    "devices_any_order": ["--devices", "0,0", "--any-order"],
    "split_input": ["--devices", "0,0", "--split-input"],
    "window1": ["--window-mb", "1"],
}
TRACE_LINE = "xz SAM on the device:"
HOST_LINE = "block(s): read on the host"


def run_cli(args, force=None):
    env = dict(os.environ, SLIMM_TRACE="cli")
    env.pop("SLIMM_FORCE", None)
    if force:
        env["SLIMM_FORCE"] = force
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def plain_run(tmp_path, w, text, extra):
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    open(sam, "wb").write(text)
    base = ["-w", str(w.options.bin_width), "-ro", "-co"] + extra
    plain_dir = str(tmp_path / "plain") + "/"
    os.makedirs(plain_dir)
    run_cli(base + ["-o", plain_dir, db, sam])
    return db, base, outputs(plain_dir, "x")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_xz_sam_writes_the_files_of_the_plain_sam(tmp_path, mode):
    grouped = "any_order" not in mode
    tag = "grouped" if grouped else "any"
    for n, kind in ((3_000, "mt"), (1_000, "two_streams_padded")):
        w = X.case_workload(grouped, n)
        text = X.case_text(tmp_path, grouped, n)
        blob = X.golden(X.GOLDEN_KINDS["mt"][1].format(tag)) if kind == "mt" else X.written_copies(text, tag)[kind]
        d = str(tmp_path / kind)
        os.makedirs(d)
        db, base, want = plain_run(tmp_path / kind, w, text, MODES[mode])
        inp = os.path.join(d, "x.sam.xz")
        open(inp, "wb").write(blob)
        # (14 blocks and three: the device takes them when told that three are enough -- 16 unless told)
        err = run_cli(base + [db, inp], force="xz_device_blocks=3" + (",xz_round=20000" if mode == "window1" else ""))
        assert outputs(d, "x.sam.xz") == want, (kind, mode)   # (_raw.tsv, the coverage files, the profile: byte for byte)
        assert (TRACE_LINE in err) == (mode != "host_decode"), (kind, mode, err[-1500:])
        assert HOST_LINE not in err, (kind, mode, err[-1500:])
        if mode != "host_decode":
            line = [ln for ln in err.split("\n") if TRACE_LINE in ln][0]
            c = X.census(blob)
            assert f"{c['streams']} streams, {c['blocks']} blocks, {len(text)} bytes of text" in line, line
        if mode == "split_input":
            assert "an xz stream is not cut by byte range; member 0 reads" in err, err[-1500:]


@pytest.mark.parametrize("grouped", [True, False])
def test_a_file_of_few_blocks_is_read_on_the_host_unless_told_otherwise(tmp_path, grouped):
    tag = "grouped" if grouped else "any"
    n, name = X.GOLDEN_KINDS["one"]
    w = X.case_workload(grouped, n)
    text = X.case_text(tmp_path, grouped, n)
    db, base, want = plain_run(tmp_path, w, text, [] if grouped else ["--any-order"])
    for force, on_device in ((None, False), ("xz_device_blocks=1", True)):
        d = str(tmp_path / ("device" if on_device else "host"))
        os.makedirs(d)
        inp = os.path.join(d, "x.sam.xz")
        open(inp, "wb").write(X.golden(name.format(tag)))
        err = run_cli(base + [db, inp], force=force)
        assert outputs(d, "x.sam.xz") == want, force
        assert (TRACE_LINE in err) == on_device and ("xz SAM of 1 " + HOST_LINE in err) == (not on_device), (force, err[-1500:])
    if grouped:   # (the default: fewer than 16 blocks)
        w, text = X.case_workload(True, 3_000), X.case_text(tmp_path, True, 3_000)
        os.makedirs(tmp_path / "mt")
        db, base, want = plain_run(tmp_path / "mt", w, text, [])
        inp = str(tmp_path / "mt" / "x.sam.xz")
        open(inp, "wb").write(X.golden(X.GOLDEN_KINDS["mt"][1].format(tag)))
        err = run_cli(base + [db, inp])
        assert outputs(str(tmp_path / "mt"), "x.sam.xz") == want
        assert TRACE_LINE not in err and "xz SAM of 14 " + HOST_LINE in err, err[-1500:]
