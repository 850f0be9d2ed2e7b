"""The `slimm` command on lz4 copies of a SAM file, on a real MI355X: a regular lz4 file's bytes go to the device
(slimm_push_lz4_sam_bytes) and every output file is the plain file's; --host-decode keeps the host reader; a group reads the
file through member 0, with --split-input too.  SLIMM_TRACE=cli says which of the two read the file.  The inputs: the committed
files of tests/golden/lz4 and frames written in Python (tests/sam_lz4.py)."""
import os
import subprocess

import pytest

from tests import sam_lz4 as L
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
}
TRACE_LINE = "lz4 SAM on the device:"


def run_cli(args, force=None):
    env = dict(os.environ, SLIMM_TRACE="cli")
    env.pop("SLIMM_FORCE", None)
    if force:
        env["SLIMM_FORCE"] = force
    r = subprocess.run([CLI] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_lz4_sam_writes_the_files_of_the_plain_sam(tmp_path, mode):
    grouped = "any_order" not in mode
    tag = "grouped" if grouped else "any"
    w = L.case_workload(grouped, 3_000)
    text = L.case_text(tmp_path, grouped, 3_000)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    open(sam, "wb").write(text)
    a, b = text[:150_000], text[150_000:]
    copies = {"linked9": L.golden(f"config1_{tag}_linked9.sam.lz4"), "default": L.golden(f"config1_{tag}_default.sam.lz4"),
              "frames": L.Frame().stored(a).bytes(block_sums=True) + L.skippable() + L.Frame().bytes() + L.Frame(linked=True).packed(b).bytes(content_size=True)}
    base = ["-w", str(w.options.bin_width), "-ro", "-co"] + MODES[mode]
    plain_dir = str(tmp_path / "plain") + "/"
    os.makedirs(plain_dir)
    run_cli(base + ["-o", plain_dir, db, sam])
    want = outputs(plain_dir, "x")
    for kind, blob in copies.items():
        d = str(tmp_path / kind)
        os.makedirs(d)
        inp = os.path.join(d, "x.sam.lz4")
        open(inp, "wb").write(blob)
        err = run_cli(base + [db, inp], force="lz4_round=20000" if mode == "window1" else None)
        assert outputs(d, "x.sam.lz4") == want, (kind, mode)   # (_raw.tsv, the coverage files, the profile: byte for byte)
        assert (TRACE_LINE in err) == (mode != "host_decode"), (kind, mode, err[-1500:])
        if mode != "host_decode":
            line = [ln for ln in err.split("\n") if TRACE_LINE in ln][0]
            c = L.census(blob)
            assert f"{c['frames']} frames, {c['stored'] + c['compressed']} blocks, {len(text)} bytes of text" in line, line
        if mode == "split_input":
            assert "an lz4 stream is not cut by byte range; member 0 reads" in err, err[-1500:]


def test_cli_damaged_lz4_fails_in_the_host_readers_words(tmp_path):
    """The device path and --host-decode say the same of a damaged file."""
    w = L.case_workload(True, 3_000)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    blob = bytearray(L.golden("config1_grouped_linked9.sam.lz4"))
    blob[L.walk(bytes(blob))[0]["blocks"][5]["at"] + 50] ^= 4
    inp = str(tmp_path / "x.sam.lz4")
    open(inp, "wb").write(bytes(blob))
    said = []
    for extra in ([], ["--host-decode"]):
        r = subprocess.run([CLI, "-w", str(w.options.bin_width)] + extra + [db, inp], capture_output=True, text=True)
        assert "block checksum mismatch" in r.stderr and "0 SAM/BAM alignment records" in r.stderr, r.stderr[-1500:]   # (the command goes on to its next file)
        said.append([ln for ln in r.stderr.split("\n") if "lz4-compressed input is not supported" in ln][0].split("lz4-compressed")[1])
    assert said[0] == said[1], said
