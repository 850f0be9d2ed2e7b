"""`slimm --devices ... --split-input` on bzip2-compressed SAM, on a real MI355X: every member of the group reads its own byte
range of the file plus the slack behind it, finds and decodes the blocks that start in its range, and the cuts are stitched
(include/slimm_hip.h, "bzip2 SAM by byte range").  The counterpart of tests/test_cli_split_input_sam.py: the files must be the
ones one device writes; a wrong first block must fall back to member 0; one device must take a file of more records than
one context holds; --host-decode keeps today's path."""
import os

import pytest

from oracle.binding import Oracle
from tests.bam_io import write_sam, write_sldb
from tests.cases import holes_case, tiny_case
from tests.helpers import assert_profiles_match
from tests.sam_bz2 import magics, one_stream, streams
from tests.test_cli_gpu import run_cli, with_names
from tests.test_cli_split_input import OUTPUTS, config1, members_of

pytestmark = pytest.mark.gpu

STEM = "sample.sam.bz2"   # (only .sam / .bam are taken off the name)
KINDS = {
    "level1": lambda text: one_stream(text, 1),                                          # one stream: every cut lies inside it
    "streams": lambda text: streams(text, chunk=max(1, len(text) // 23 + 1), levels=(1, 9, 5, 2), empty_at=2),   # (as pbzip2 writes)
}


def write_input(tmp_path, w, kind):
    db = str(tmp_path / "db.sldb")
    inp = str(tmp_path / STEM)
    if not os.path.exists(db):
        write_sldb(db, w.taxonomy)
        sam = str(tmp_path / "text.sam")
        write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
        open(inp, "wb").write(KINDS[kind](open(sam, "rb").read()))
        os.remove(sam)   # (the command is given one file)
    return db, inp


def files_of(tmp_path, w, kind, tag, extra, env=None):
    db, inp = write_input(tmp_path, w, kind)
    out = str(tmp_path / tag) + "/"
    os.makedirs(out)
    e = dict(os.environ, SLIMM_TRACE="cli")
    e.update(env or {})
    err = run_cli(["-w", str(w.options.bin_width), "-o", out, "-ro", "-co", "-v"] + extra + [db, inp], env=e)
    return {s: open(os.path.join(out, STEM + s + ".tsv")).read() for s in OUTPUTS}, err


def split_matches_one_device(tmp_path, w, kind, devices, env=None, extra=(), fallback=False):
    one, _ = files_of(tmp_path, w, kind, "one", [])
    got, err = files_of(tmp_path, w, kind, "split", ["--devices", devices, "--split-input", "--window-mb", "1"] + list(extra), env=env)
    assert got == one
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=False)
    assert_profiles_match(got["_profile"], o.profile_tsv)
    assert ("device decode on member 0" in err) == fallback, err[-3000:]   # (today's path: member 0 reads the whole file)
    return err


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
@pytest.mark.parametrize("mk", [tiny_case, holes_case, config1], ids=["tiny", "holes", "config1"])
def test_split_input_writes_the_single_device_files(tmp_path, mk, devices, kind):
    err = split_matches_one_device(tmp_path, with_names(mk()), kind, devices)
    assert "split input:" not in err, err[-2000:]
    ms = members_of(err)
    assert len(ms) == devices.count("0")                       # every member reports its share
    assert [m[1] for m in ms[1:]] == [m[2] for m in ms[:-1]] and ms[0][1] == 0 and ms[-1][2] == ms[0][3]
    assert sum(m[4] for m in ms) > 0
    assert "is not cut by byte range" not in err


def test_split_input_every_member_decodes_blocks_of_its_own(tmp_path):
    w = with_names(config1())
    err = split_matches_one_device(tmp_path, w, "streams", "0,0,0,0")
    blob = open(str(tmp_path / STEM), "rb").read()
    ms = members_of(err)
    bits = magics(blob)
    assert len(bits) >= 8
    for _, lo, hi, total, records in ms:
        assert total == len(blob)
        assert any(lo * 8 <= b < hi * 8 for b in bits) and records > 0, ms


def test_split_input_wrong_first_block_falls_back_to_member_0(tmp_path):
    err = split_matches_one_device(tmp_path, with_names(config1()), "streams", "0,0,0", env={"SLIMM_FORCE": "bzip2_split_wrong_first"},
                                   fallback=True)
    assert "split input:" in err and "reading the file through member 0" in err


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_device_takes_more_records_than_one_context(tmp_path, kind):
    """SLIMM_FORCE record_cap: a context takes a third of the file's records; contexts of a group on the one device read a
    byte range each."""
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, kind, "one", [])
    n = len(w.records.read_key)
    got, err = files_of(tmp_path, w, kind, "capped", ["--window-mb", "1"], env={"SLIMM_FORCE": f"record_cap={n // 3}"})
    assert got == one
    assert "reading the file by byte range" in err
    assert len(members_of(err)) >= 4 and "decoding on the host" not in err


def test_host_decode_with_split_input_keeps_todays_path(tmp_path):
    """--host-decode reads the file with the host's serial decoder and deals the records: nothing is read by byte range."""
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, "streams", "one", [])
    got, err = files_of(tmp_path, w, "streams", "host", ["--devices", "0,0", "--split-input", "--host-decode"])
    assert got == one
    assert not members_of(err) and "split input:" not in err
