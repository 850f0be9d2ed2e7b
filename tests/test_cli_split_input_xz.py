"""`slimm --devices ... --split-input` on xz-compressed SAM of several blocks, on a real MI355X: every member of the group
reads exactly its own byte range of the file -- cut where its index says a block starts (slimm_host_xz_ranges) --, is told
the check kind of the stream around its range, decodes its blocks, and the cuts are stitched (include/slimm_hip.h, "xz SAM by
byte range").  The counterpart of tests/test_cli_split_input_zstd.py: every output file must be the plain SAM's, byte for
byte; below the floor (slimm_xz_split_floor: SLIMM_FORCE xz_split_blocks=N lowers it here, xz_device_blocks does not) member 0
reads, and says so; one device must take a file of more records than one context holds.  The input: the committed file of 14
blocks (tests/golden/xz)."""
import os

import pytest

from tests import sam_xz as X
from tests.test_cli_split_input import members_of
from tests.test_cli_xz_sam_device import TRACE_LINE, plain_run, run_cli
from tests.test_gpu_compressed_sam import outputs

pytestmark = pytest.mark.gpu

DEVICE = "xz_device_blocks=3"          # (14 blocks: the device reads the file at all -- 16 unless told)
CUT = DEVICE + ",xz_split_blocks=2"    # (... and is cut for two or three members: 13 blocks behind the header's)
NOT_CUT = "an xz stream is not cut by byte range; member 0 reads"


def run_on_the_golden(tmp_path, grouped, extra, force, tag):
    """(the plain SAM's files, this run's files, its trace, the xz file's bytes)"""
    w, text = X.case_workload(grouped, 3_000), X.case_text(tmp_path, grouped, 3_000)
    blob = X.golden(X.GOLDEN_KINDS["mt"][1].format("grouped" if grouped else "any"))
    d = tmp_path / tag
    os.makedirs(d)
    db, base, want = plain_run(d, w, text, [] if grouped else ["--any-order"])
    inp = str(d / "x.sam.xz")
    open(inp, "wb").write(blob)
    err = run_cli(base + extra + [db, inp], force=force)
    return want, outputs(str(d), "x.sam.xz"), err, blob


def check_members_and_census(err, blob, n_members):
    assert "split input:" not in err and NOT_CUT not in err and "device decode on member 0" not in err, err[-2000:]
    ms = members_of(err)
    assert len(ms) == n_members                                # one line per member
    assert [m[1] for m in ms[1:]] == [m[2] for m in ms[:-1]] and ms[0][1] == 0 and ms[-1][2] == ms[0][3] == len(blob)
    blocks = [b["at"] for b in X.walk(blob)[0]["blocks"]]
    assert all(m[1] in blocks[1:] for m in ms[1:]) and all(any(m[1] <= at < m[2] for at in blocks) and m[4] > 0 for m in ms)
    lines = [ln for ln in err.split("\n") if TRACE_LINE in ln]
    c = X.census(blob)
    assert len(lines) == 1 and f"{c['streams']} streams, {c['blocks']} blocks, {c['text']} bytes of text" in lines[0], lines


@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "any_order"])
def test_split_input_writes_the_files_of_the_plain_sam(tmp_path, grouped, devices):
    want, got, err, blob = run_on_the_golden(tmp_path, grouped, ["--devices", devices, "--split-input"], CUT, "split")
    assert got == want
    check_members_and_census(err, blob, devices.count("0"))
    assert ("dealt by key" in err) == (not grouped)


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "any_order"])
def test_below_the_floor_member_0_reads_and_says_so(tmp_path, grouped):
    """Without SLIMM_FORCE xz_split_blocks the floor is 16 blocks a member, whatever xz_device_blocks says: 13 / 2 are fewer."""
    want, got, err, blob = run_on_the_golden(tmp_path, grouped, ["--devices", "0,0", "--split-input"], DEVICE, "floor")
    assert got == want
    assert not members_of(err) and "split input:" not in err
    assert TRACE_LINE in err and NOT_CUT in err, err[-2000:]
    # ... and a file the host reader takes is not cut either, whatever the floor
    want, got, err, blob = run_on_the_golden(tmp_path, grouped, ["--devices", "0,0", "--split-input"], "xz_split_blocks=2", "host")
    assert got == want
    assert not members_of(err) and TRACE_LINE not in err and "xz SAM of 14 block(s): read on the host" in err, err[-2000:]


def test_one_device_takes_more_records_than_one_context(tmp_path):
    """SLIMM_FORCE record_cap: a context takes a third of the file's records; contexts of a group on the one device read a
    byte range each.  The floor is not asked for here."""
    want, got, err, blob = run_on_the_golden(tmp_path, True, ["--window-mb", "1"], DEVICE + ",record_cap=1000", "capped")
    assert got == want
    assert "reading the file by byte range" in err
    assert len(members_of(err)) >= 4 and "decoding on the host" not in err
