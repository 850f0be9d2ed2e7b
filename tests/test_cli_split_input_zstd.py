"""`slimm --devices ... --split-input` on zstd-compressed SAM of several frames, on a real MI355X: every member of the group
reads exactly its own byte range of the file -- cut where frames start (slimm_host_zstd_ranges) --, decodes its frames, and
the cuts are stitched (include/slimm_hip.h, "zstd SAM by byte range").  The counterpart of
tests/test_cli_split_input_bzip2.py: the files must be the ones one device writes; a wrong cut must fall back to member 0;
one device must take a file of more records than one context holds; a file of one frame, a file below the floor
(slimm_zstd_split_floor: SLIMM_FORCE zstd_split_floor=0 lowers it here) and --host-decode keep today's path."""
import os

import pytest

from oracle.binding import Oracle
from slimm_amd.synth import CONFIGS, make_workload
from tests import sam_zst as Z
from tests.bam_io import write_sam, write_sldb
from tests.cases import holes_case, tiny_case
from tests.helpers import assert_profiles_match
from tests.test_cli_gpu import run_cli, with_names
from tests.test_cli_split_input import OUTPUTS, config1, members_of

pytestmark = pytest.mark.gpu

STEM = "sample.sam.zst"   # (only .sam / .bam are taken off the name)
FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_frames")
UNSORTED = "@HD\tVN:1.6\tSO:unsorted"
NO_FLOOR = "zstd_split_floor=0"
NOT_CUT = "a zstd stream is not cut by byte range; member 0 reads"
TRACE_LINE = "zstd SAM on the device:"


def frames_of(text, step=0):
    """frames of `step` bytes of text in raw blocks (cut inside lines; 30 000 bytes, or 1 500 of a text too short for several
    of those), an empty frame and two skippable frames among them"""
    step = step or (30_000 if len(text) > 200_000 else 1_500)
    out = []
    for k, i in enumerate(range(0, len(text), step)):
        out.append(Z.raw_frame(text[i:i + step], step=step))
        if k == 1:
            out.append(Z.raw_frame(b""))
        if k in (0, 2):
            out.append(Z.skippable())
    return b"".join(out)


KINDS = {"frames": frames_of, "one_frame": lambda text: Z.raw_frame(text)}


def shuffled():
    return make_workload(CONFIGS["config1"], seed=45, n_records=4000, shuffled=True)


def write_input(tmp_path, w, kind, hd=None):
    db = str(tmp_path / "db.sldb")
    inp = str(tmp_path / STEM)
    if not os.path.exists(db):
        write_sldb(db, w.taxonomy)
        sam = str(tmp_path / "text.sam")
        write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, **({"hd": hd} if hd else {}))
        open(inp, "wb").write(KINDS[kind](open(sam, "rb").read()))
        os.remove(sam)   # (the command is given one file)
    return db, inp


def run_to(tmp_path, w, db, inp, tag, extra, force):
    out = str(tmp_path / tag) + "/"
    os.makedirs(out)
    e = dict(os.environ, SLIMM_TRACE="cli")
    e.pop("SLIMM_FORCE", None)
    if force:
        e["SLIMM_FORCE"] = force
    err = run_cli(["-w", str(w.options.bin_width), "-o", out, "-ro", "-co", "-v"] + extra + [db, inp], env=e)
    return {s: open(os.path.join(out, STEM + s + ".tsv")).read() for s in OUTPUTS}, err


def files_of(tmp_path, w, kind, tag, extra, force=NO_FLOOR, hd=None):
    db, inp = write_input(tmp_path, w, kind, hd)
    return run_to(tmp_path, w, db, inp, tag, extra, force)


def split_matches_one_device(tmp_path, w, kind, devices, force=NO_FLOOR, extra=(), fallback=False, hd=None):
    one, _ = files_of(tmp_path, w, kind, "one", list(extra), hd=hd)
    got, err = files_of(tmp_path, w, kind, "split", ["--devices", devices, "--split-input", "--window-mb", "1"] + list(extra), force=force, hd=hd)
    assert got == one
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=False)
    assert_profiles_match(got["_profile"], o.profile_tsv)
    assert ("device decode on member 0" in err) == fallback, err[-3000:]   # (today's path: member 0 reads the whole file)
    return err


def check_members_and_census(tmp_path, err, n_members):
    blob = open(str(tmp_path / STEM), "rb").read()
    assert "split input:" not in err, err[-2000:]
    ms = members_of(err)
    assert len(ms) == n_members                                # one line per member
    assert [m[1] for m in ms[1:]] == [m[2] for m in ms[:-1]] and ms[0][1] == 0 and ms[-1][2] == ms[0][3] == len(blob)
    starts = {f["at"] for f in Z.walk(blob)} | {len(blob)}
    assert all(m[1] in starts for m in ms[1:])
    assert sum(m[4] for m in ms) > 0
    assert NOT_CUT not in err
    lines = [ln for ln in err.split("\n") if TRACE_LINE in ln]
    c = Z.census(blob)
    text_bytes = sum(b["size"] for f in Z.walk(blob) for b in f["blocks"])   # (raw and RLE blocks: their size is their text's)
    assert len(lines) == 1 and f"{c['frames']} frames, {c['raw'] + c['rle'] + c['compressed']} blocks, {text_bytes} bytes of text" in lines[0], lines


@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
@pytest.mark.parametrize("mk", [tiny_case, holes_case, config1], ids=["tiny", "holes", "config1"])
def test_split_input_writes_the_single_device_files(tmp_path, mk, devices):
    err = split_matches_one_device(tmp_path, with_names(mk()), "frames", devices)
    check_members_and_census(tmp_path, err, devices.count("0"))


@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
def test_split_input_on_a_file_in_any_order(tmp_path, devices):
    err = split_matches_one_device(tmp_path, with_names(shuffled()), "frames", devices, extra=["--any-order"], hd=UNSORTED)
    check_members_and_census(tmp_path, err, devices.count("0"))
    assert "dealt by key" in err


def test_split_input_every_member_decodes_frames_of_its_own(tmp_path):
    w = with_names(config1())
    err = split_matches_one_device(tmp_path, w, "frames", "0,0,0,0")
    blob = open(str(tmp_path / STEM), "rb").read()
    frames = [f["at"] for f in Z.walk(blob) if not f["skippable"]]
    for _, lo, hi, total, records in members_of(err):
        assert total == len(blob)
        assert any(lo <= at < hi for at in frames) and records > 0


def test_a_file_of_one_frame_goes_through_member_0(tmp_path):
    err = split_matches_one_device(tmp_path, with_names(config1()), "one_frame", "0,0", fallback=True)
    assert NOT_CUT in err and not members_of(err) and "split input:" not in err


def test_the_floor_keeps_a_small_file_with_member_0(tmp_path):
    """Without SLIMM_FORCE zstd_split_floor: the committed file of seven frames is 27 582 bytes, far below 32 MiB a member."""
    w = Z.case_workload(True, 3_000)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    inp = os.path.join(FRAMES, "config1_grouped_frames_l3.sam.zst")
    out = {}
    for tag, force in (("floor", None), ("cut", NO_FLOOR)):
        d = str(tmp_path / tag) + "/"
        os.makedirs(d)
        e = dict(os.environ, SLIMM_TRACE="cli")
        e.pop("SLIMM_FORCE", None)
        if force:
            e["SLIMM_FORCE"] = force
        err = run_cli(["-w", str(w.options.bin_width), "-o", d, "-ro", "-co", "--devices", "0,0", "--split-input", db, inp], env=e)
        out[tag] = {s: open(os.path.join(d, os.path.basename(inp) + s + ".tsv")).read() for s in OUTPUTS}
        assert (NOT_CUT in err) == (force is None), err[-2000:]
        assert ("device decode on member 0" in err) == (force is None)
        assert len(members_of(err)) == (0 if force is None else 2)
        assert "14 frames" not in err and "7 frames, 7 blocks, 445770 bytes of text" in err
    assert out["floor"] == out["cut"]


def test_split_input_wrong_cut_falls_back_to_member_0(tmp_path):
    err = split_matches_one_device(tmp_path, with_names(config1()), "frames", "0,0", force=NO_FLOOR + ",zstd_split_wrong_cut", fallback=True)
    assert "split input:" in err and "reading the file through member 0" in err
    os.makedirs(tmp_path / "four")
    err = split_matches_one_device(tmp_path / "four", with_names(config1()), "frames", "0,0,0,0", force=NO_FLOOR + ",zstd_split_wrong_cut",
                                   fallback=True)
    assert "split input:" in err and "reading the file through member 0" in err


def test_one_device_takes_more_records_than_one_context(tmp_path):
    """SLIMM_FORCE record_cap: a context takes a third of the file's records; contexts of a group on the one device read a
    byte range each.  The floor is not asked for here.  A file of one frame cannot be cut: it fails at the cap as before."""
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, "frames", "one", [])
    n = len(w.records.read_key)
    got, err = files_of(tmp_path, w, "frames", "capped", ["--window-mb", "1"], force=f"record_cap={n // 3}")
    assert got == one
    assert "reading the file by byte range" in err
    assert len(members_of(err)) >= 4 and "decoding on the host" not in err


def test_host_decode_with_split_input_keeps_todays_path(tmp_path):
    """--host-decode reads the file with the host's serial decoder and deals the records: nothing is read by byte range."""
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, "frames", "one", [])
    got, err = files_of(tmp_path, w, "frames", "host", ["--devices", "0,0", "--split-input", "--host-decode"])
    assert got == one
    assert not members_of(err) and "split input:" not in err and TRACE_LINE not in err
