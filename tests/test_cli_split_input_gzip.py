"""`slimm --devices ... --split-input` on gzip-compressed SAM, on a real MI355X: every member of the group reads the bytes that
hold its own bit range of the file -- cut where dynamic blocks start (slimm_host_gzip_ranges) -- twice, the window pass and
the text pass, and the cuts are stitched (include/slimm_hip.h, "gzip SAM by byte range").  The counterpart of
tests/test_cli_split_input_bzip2.py: the files must be the ones one device writes; a wrong cut must fall back to member 0;
one device must take a file of more records than one context holds; a file below the floor (slimm_gzip_split_floor:
SLIMM_FORCE gzip_split_floor=0 lowers it here) keeps today's path and today's trace line."""
import os

import pytest

from oracle.binding import Oracle
from slimm_amd.synth import CONFIGS, make_workload
from tests import sam_deflate as D
from tests.bam_io import write_sam, write_sldb
from tests.helpers import assert_profiles_match
from tests.test_cli_gpu import run_cli, with_names
from tests.test_cli_split_input import OUTPUTS, members_of
from tests.test_split_gzip_plan import file_blocks

pytestmark = pytest.mark.gpu

STEM = "sample.sam.gz"   # (only .sam / .bam are taken off the name)
UNSORTED = "@HD\tVN:1.6\tSO:unsorted"
NO_FLOOR = "gzip_chunk=2048,gzip_split_floor=0"
NOT_CUT = "--split-input: a gzip stream is not cut by byte range; member 0 reads"
WINDOW_PASS = "gzip window pass:"


def config1():
    return make_workload(CONFIGS["config1"], seed=41, n_records=4000)


def shuffled():
    return make_workload(CONFIGS["config1"], seed=45, n_records=4000, shuffled=True)


def write_input(tmp_path, w, hd=None):
    db = str(tmp_path / "db.sldb")
    inp = str(tmp_path / STEM)
    if not os.path.exists(db):
        write_sldb(db, w.taxonomy)
        sam = str(tmp_path / "text.sam")
        write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, **({"hd": hd} if hd else {}))
        open(inp, "wb").write(D.member(open(sam, "rb").read(), memLevel=1))   # (one gzip member of many dynamic blocks)
        os.remove(sam)   # (the command is given one file)
    return db, inp


def files_of(tmp_path, w, tag, extra, force=NO_FLOOR, hd=None):
    db, inp = write_input(tmp_path, w, hd)
    out = str(tmp_path / tag) + "/"
    os.makedirs(out)
    e = dict(os.environ, SLIMM_TRACE="cli")
    e.pop("SLIMM_FORCE", None)
    if force:
        e["SLIMM_FORCE"] = force
    err = run_cli(["-w", str(w.options.bin_width), "-o", out, "-ro", "-co", "-v"] + extra + [db, inp], env=e)
    return {s: open(os.path.join(out, STEM + s + ".tsv")).read() for s in OUTPUTS}, err


def split_matches_one_device(tmp_path, w, devices, force=NO_FLOOR, extra=(), fallback=False, hd=None):
    one, _ = files_of(tmp_path, w, "one", list(extra), hd=hd)
    got, err = files_of(tmp_path, w, "split", ["--devices", devices, "--split-input", "--window-mb", "1"] + list(extra), force=force, hd=hd)
    assert got == one
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=False)
    assert_profiles_match(got["_profile"], o.profile_tsv)
    assert ("device decode on member 0" in err) == fallback, err[-3000:]   # (today's path: member 0 reads the whole file)
    return err


def check_members(tmp_path, err, n_members):
    blob = open(str(tmp_path / STEM), "rb").read()
    assert "split input:" not in err, err[-2000:]
    ms = members_of(err)
    assert len(ms) == n_members                                # one line per member: the text pass's
    assert ms[0][1] == 0 and ms[-1][2] == ms[0][3] == len(blob)
    assert all(b[1] in (a[2], a[2] - 1) for a, b in zip(ms, ms[1:]))   # (neighbours share at most one byte)
    assert sum(m[4] for m in ms) > 0 and all(m[4] > 0 for m in ms)
    assert NOT_CUT not in err
    assert len([ln for ln in err.split("\n") if WINDOW_PASS in ln]) == 1
    lines = [ln for ln in err.split("\n") if "gzip SAM on the device:" in ln]
    text_bytes = sum(b[3] for b in file_blocks(blob))
    assert len(lines) == 1 and f"1 members, " in lines[0] and f"{text_bytes} bytes of text" in lines[0], lines


@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
def test_split_input_writes_the_single_device_files(tmp_path, devices):
    err = split_matches_one_device(tmp_path, with_names(config1()), devices)
    check_members(tmp_path, err, devices.count("0"))


def test_split_input_on_a_file_in_any_order(tmp_path):
    err = split_matches_one_device(tmp_path, with_names(shuffled()), "0,0,0,0", extra=["--any-order"], hd=UNSORTED)
    check_members(tmp_path, err, 4)
    assert "dealt by key" in err


def test_the_floor_keeps_a_small_file_with_member_0(tmp_path):
    """Without SLIMM_FORCE gzip_split_floor the same file -- some 100 KB -- is far below 32 MiB a member: today's path, today's line."""
    err = split_matches_one_device(tmp_path, with_names(config1()), "0,0,0,0", force="gzip_chunk=2048", fallback=True)
    assert NOT_CUT in err and not members_of(err) and "split input:" not in err and WINDOW_PASS not in err


def test_split_input_wrong_cut_falls_back_to_member_0(tmp_path):
    err = split_matches_one_device(tmp_path, with_names(config1()), "0,0,0", force=NO_FLOOR + ",gzip_split_wrong_cut", fallback=True)
    assert "split input:" in err and "reading the file through member 0" in err


def test_one_device_takes_more_records_than_one_context(tmp_path):
    """SLIMM_FORCE record_cap: a context takes a third of the file's records; contexts of a group on the one device read a
    range each.  The floor is not asked there."""
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, "one", [], force="gzip_chunk=2048")
    n = len(w.records.read_key)
    got, err = files_of(tmp_path, w, "capped", ["--window-mb", "1"], force=f"gzip_chunk=2048,record_cap={n // 3}")
    assert got == one
    assert "reading the file by byte range" in err
    assert len(members_of(err)) >= 4 and "decoding on the host" not in err


def test_host_decode_with_split_input_keeps_todays_path(tmp_path):
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, "one", [])
    got, err = files_of(tmp_path, w, "host", ["--devices", "0,0", "--split-input", "--host-decode"])
    assert got == one
    assert not members_of(err) and "split input:" not in err and WINDOW_PASS not in err
