"""The `slimm` command on zstd copies of a SAM file, on a real MI355X: a regular zstd file's bytes go to the device
(slimm_push_zstd_sam_bytes) and every output file is the plain file's; --host-decode keeps the host reader; a group reads
the file through member 0, with --split-input too.  SLIMM_TRACE=cli says which of the two read the file.  The inputs: the
committed files of tests/golden/zstd and frames written in Python (tests/sam_zst.py)."""
import os
import subprocess

import pytest

from tests import sam_zst as Z
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
TRACE_LINE = "zstd SAM on the device:"


def run_cli(args, force=None):
    env = dict(os.environ, SLIMM_TRACE="cli")
    env.pop("SLIMM_FORCE", None)
    if force:
        env["SLIMM_FORCE"] = force
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_zstd_sam_writes_the_files_of_the_plain_sam(tmp_path, mode):
    grouped = "any_order" not in mode
    tag = "grouped" if grouped else "any"
    w = Z.case_workload(grouped, 3_000)
    text = Z.case_text(tmp_path, grouped, 3_000)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    open(sam, "wb").write(text)
    copies = {"l19": Z.golden(f"config1_{tag}_l19.sam.zst"), "frames": Z.written_copies(text)["frames"]}
    base = ["-w", str(w.options.bin_width), "-ro", "-co"] + MODES[mode]
    plain_dir = str(tmp_path / "plain") + "/"
    os.makedirs(plain_dir)
    run_cli(base + ["-o", plain_dir, db, sam])
    want = outputs(plain_dir, "x")
    for kind, blob in copies.items():
        d = str(tmp_path / kind)
        os.makedirs(d)
        inp = os.path.join(d, "x.sam.zst")
        open(inp, "wb").write(blob)
        err = run_cli(base + [db, inp], force="zstd_round=20000" if mode == "window1" else None)
        assert outputs(d, "x.sam.zst") == want, (kind, mode)   # (_raw.tsv, the coverage files, the profile: byte for byte)
        assert (TRACE_LINE in err) == (mode != "host_decode"), (kind, mode, err[-1500:])
        if mode != "host_decode":
            line = [ln for ln in err.split("\n") if TRACE_LINE in ln][0]
            c = Z.census(blob)
            assert f"{c['frames']} frames, {c['raw'] + c['rle'] + c['compressed']} blocks, {len(text)} bytes of text" in line, line
        if mode == "split_input":
            assert "a zstd stream is not cut by byte range; member 0 reads" in err, err[-1500:]
