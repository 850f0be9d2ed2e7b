"""The `slimm` command on lzip copies of a SAM file, on a real MI355X: a regular lzip file of 16 members or more goes to the
device (slimm_push_lzip_sam_bytes; SLIMM_TRACE=push shows `[push lzip]`) and every output file is the plain file's; a file of
fewer members, counted by its trailers (slimm_host_lzip_members), goes to the host reader unless SLIMM_FORCE
lzip_device_members says otherwise; --host-decode keeps the host reader; a group reads the file through member 0, with
--split-input too; the record filter applies.  The inputs: the committed files of tests/golden/lzip (tests/sam_lzip.py)."""
import os
import subprocess

import pytest

from tests import sam_lzip as Z
from tests.bam_io import write_sldb
from tests.test_gpu_compressed_sam import CLI, outputs

pytestmark = pytest.mark.gpu

MODES = {
    "device": [],
    "host_decode": ["--host-decode"],
    "any_order": ["--any-order"],
    "devices": ["--devices", "0,0"],
    "split_input": ["--devices", "0,0", "--split-input"],
    "window1": ["--window-mb", "1"],
    "filter": ["-q", "30"],
}
TRACE_LINE = "lzip SAM on the device:"


def run_cli(args, force=None):
    env = dict(os.environ, SLIMM_TRACE="cli,push")
    env.pop("SLIMM_FORCE", None)
    if force:
        env["SLIMM_FORCE"] = force
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def plain_run(tmp_path, w, text, base):
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    open(sam, "wb").write(text)
    plain_dir = str(tmp_path / "plain") + "/"
    os.makedirs(plain_dir)
    run_cli(base + ["-o", plain_dir, db, sam])
    return db, outputs(plain_dir, "x")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_lzip_sam_of_17_members_takes_the_device_and_writes_the_files_of_the_plain_sam(tmp_path, mode):
    grouped = "any_order" not in mode
    tag = "grouped" if grouped else "any"
    w = Z.case_workload(grouped, 3_000)
    text = Z.case_text(tmp_path, grouped, 3_000)
    base = ["-w", str(w.options.bin_width), "-ro", "-co"] + MODES[mode]
    db, want = plain_run(tmp_path, w, text, base)   # (with the filter: the filtered plain SAM run)
    blob = Z.golden(f"config1_{tag}_m17.sam.lz")
    d = str(tmp_path / "m17")
    os.makedirs(d)
    inp = os.path.join(d, "x.sam.lz")
    open(inp, "wb").write(blob)
    err = run_cli(base + [db, inp], force="lzip_round=2000" if mode == "window1" else None)
    assert outputs(d, "x.sam.lz") == want, mode   # (_raw.tsv, the coverage files, the profile: byte for byte)
    on_device = mode != "host_decode"
    assert (TRACE_LINE in err) == on_device and ("[push lzip]" in err) == on_device, (mode, err[-1500:])
    if on_device:
        line = [ln for ln in err.split("\n") if TRACE_LINE in ln][0]
        assert f"17 members, {len(text)} bytes of text" in line, line
    if mode == "split_input":
        assert "an lzip stream is not cut by byte range; member 0 reads" in err, err[-1500:]


def test_cli_a_file_of_one_member_goes_to_the_host_reader_unless_forced(tmp_path):
    w = Z.case_workload(True, 1_000)
    text = Z.case_text(tmp_path, True, 1_000)
    base = ["-w", str(w.options.bin_width), "-ro", "-co"]
    db, want = plain_run(tmp_path, w, text, base)
    for force, on_device in ((None, False), ("lzip_device_members=1", True), ("lzip_device_members=2", False)):
        d = str(tmp_path / f"one_{on_device}_{force}")
        os.makedirs(d)
        inp = os.path.join(d, "x.sam.lz")
        open(inp, "wb").write(Z.golden("short_grouped_one.sam.lz"))
        err = run_cli(base + [db, inp], force=force)
        assert outputs(d, "x.sam.lz") == want, force
        assert ("[push lzip]" in err) == on_device and ("lzip SAM of 1 member(s): read on the host" in err) != on_device, (force, err[-1500:])


def test_cli_damaged_lzip_fails_in_the_host_readers_words(tmp_path):
    """The device path and --host-decode say the same of a damaged file."""
    w = Z.case_workload(True, 3_000)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    blob = bytearray(Z.golden("config1_grouped_m17.sam.lz"))
    m = Z.walk(bytes(blob))[5]
    blob[m["stream_at"] + 50] ^= 4
    inp = str(tmp_path / "x.sam.lz")
    open(inp, "wb").write(bytes(blob))
    said = []
    for extra in ([], ["--host-decode"]):
        r = subprocess.run([CLI, "-w", str(w.options.bin_width)] + extra + [db, inp], capture_output=True, text=True)
        assert f"member at byte {m['at']}: " in r.stderr and "0 SAM/BAM alignment records" in r.stderr, r.stderr[-1500:]   # (the command goes on to its next file)
        said.append([ln for ln in r.stderr.split("\n") if "lzip-compressed input is not supported" in ln][0].split("lzip-compressed")[1])
    assert said[0] == said[1], said
