"""`slimm --devices ... --split-input` on SAM text and on BGZF blocks of it, on a real MI355X: every member of the group reads
(inflates) and decodes its own byte range of a name-grouped file and the cuts are stitched on the device (include/slimm_hip.h,
"ONE FILE SPLIT BY BYTE RANGE").  The counterpart of tests/test_cli_split_input.py, case by case: the files must be the ones
one device writes; a head that is off by a byte must fall back to member 0; one device must take a file of more records
than one context holds; a gzip stream keeps today's path."""
import os
import random
import re

import numpy as np
import pytest

from oracle.binding import Oracle
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.workload import Workload
from tests.bam_io import write_sam, write_sldb
from tests.cases import Q18_APART_EXPECTED, holes_case, q18_apart_case, records_from_sam, tiny_case
from tests.helpers import assert_profiles_match
from tests.sam_gz import bgzf, gzip_members
from tests.test_cli_gpu import check_outputs, run_cli, with_names
from tests.test_cli_split_input import OUTPUTS, config1, members_of, one_run

pytestmark = pytest.mark.gpu

FORMS = ["sam", "bgzf"]
INPUT = {"sam": "sample.sam", "bgzf": "sample.sam.gz", "gzip": "sample.sam.gz"}
STEM = {"sam": "sample", "bgzf": "sample.sam.gz", "gzip": "sample.sam.gz"}   # (only .sam / .bam are taken off the name)


def write_input(tmp_path, w, form, edit=None, blocks=(20_000, 65_000)):
    """db.sldb and the input of the form, once per directory.  edit: text -> text, applied to the SAM file's bytes"""
    db = str(tmp_path / "db.sldb")
    inp = str(tmp_path / INPUT[form])
    if not os.path.exists(db):
        write_sldb(db, w.taxonomy)
        sam = str(tmp_path / "text.sam") if form != "sam" else inp
        write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
        text = open(sam, "rb").read()
        if edit:
            text = edit(text)
            open(sam, "wb").write(text)
        if form == "bgzf":
            open(inp, "wb").write(bgzf(text, seed=7, lo=blocks[0], hi=blocks[1]))
        if form == "gzip":
            open(inp, "wb").write(gzip_members(text, 2))
        if form != "sam":
            os.remove(sam)   # (the command is given one file)
    return db, inp


def files_of(tmp_path, w, form, tag, extra, env=None, **kw):
    db, inp = write_input(tmp_path, w, form, **kw)
    out = str(tmp_path / tag) + "/"
    os.makedirs(out)
    e = dict(os.environ, SLIMM_TRACE="cli")
    e.update(env or {})
    err = run_cli(["-w", str(w.options.bin_width), "-o", out, "-ro", "-co", "-v"] + extra + [db, inp], env=e)
    return {s: open(os.path.join(out, STEM[form] + s + ".tsv")).read() for s in OUTPUTS}, err


def split_matches_one_device(tmp_path, w, form, devices, env=None, oracle=True, fallback=False, **kw):
    one, _ = files_of(tmp_path, w, form, "one", [], **kw)
    got, err = files_of(tmp_path, w, form, "split", ["--devices", devices, "--split-input", "--window-mb", "1"], env=env, **kw)
    assert got == one
    if oracle:  # (a workload built here has no oracle of its own to trust more than the single-device run)
        o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=False)
        assert_profiles_match(got["_profile"], o.profile_tsv)
    assert ("device decode on member 0" in err) == fallback, err[-3000:]   # (today's path: member 0 reads the whole file)
    return err


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0"])
@pytest.mark.parametrize("mk", [tiny_case, holes_case, config1], ids=["tiny", "holes", "config1"])
def test_split_input_writes_the_single_device_files(tmp_path, mk, devices, form):
    err = split_matches_one_device(tmp_path, with_names(mk()), form, devices)
    assert "split input:" not in err, err[-2000:]
    assert len(members_of(err)) == devices.count("0")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0", "0,0,0,0,0,0,0,0"])
def test_split_input_run_of_10000_records_across_a_cut(tmp_path, devices, form):
    w = config1()
    n = len(w.records.read_key)
    err = split_matches_one_device(tmp_path, one_run(w, n // 2 - 5000, n // 2 + 5000), form, devices, oracle=False)
    assert "split input:" not in err
    assert len(members_of(err)) == devices.count("0")
    handed = [int(x) for x in re.findall(r"handed (\d+) records left", err)]
    assert max(handed) > 1000   # (the run's part behind a cut went to the member that holds its start)


@pytest.mark.parametrize("form", FORMS)
def test_split_input_run_over_a_whole_middle_member(tmp_path, form):
    w = config1()
    n = len(w.records.read_key)
    err = split_matches_one_device(tmp_path, one_run(w, n // 8, 7 * n // 8), form, "0,0,0,0", oracle=False)
    assert "split input:" not in err
    assert re.search(r"member [12] handed \d+ records left to member 0, keeps 0", err), err[-3000:]


@pytest.mark.parametrize("form", FORMS)
def test_split_input_cuts_inside_lines(tmp_path, form):
    """Text cut anywhere: practically every range starts inside a line, whose bytes through the newline are the head."""
    err = split_matches_one_device(tmp_path, with_names(config1()), form, "0,0,0,0,0,0", oracle=False)
    assert "split input:" not in err
    assert len(members_of(err)) == 6
    heads = [int(x) for x in re.findall(r"cut in front of member \d+: (\d+) head bytes", err)]
    assert heads and max(heads) > 0


def long_line(text: bytes) -> bytes:
    """alignment line 30 gets a SEQ of 400 000 bases"""
    lines = text.splitlines(keepends=True)
    k = next(i for i, l in enumerate(lines) if not l.startswith(b"@")) + 30
    f = lines[k].split(b"\t")
    f[5], f[9] = b"400000M", b"A" * 400_000
    lines[k] = b"\t".join(f)
    return b"".join(lines)


@pytest.mark.parametrize("form", FORMS)
def test_split_input_members_without_a_line_start(tmp_path, form):
    # one line of 400 000 bases among the tiny case's, eight members: ranges that lie inside it are all head
    os.makedirs(tmp_path / "long")
    err = split_matches_one_device(tmp_path / "long", with_names(tiny_case()), form, "0,0,0,0,0,0,0,0", oracle=False, edit=long_line)
    assert "split input:" not in err
    ms = members_of(err)
    assert len(ms) == 8
    assert any(m[4] == 0 and m[2] > m[1] for m in ms), err[-3000:]
    # the tiny case alone.  BGZF: one block of alignment lines for eight members, so there are empty ranges.  Plain text is
    # cut evenly wherever the bytes are (slimm_host_text_ranges), so 74 lines leave no range empty: each has its eighth
    os.makedirs(tmp_path / "tiny")
    err = split_matches_one_device(tmp_path / "tiny", with_names(tiny_case()), form, "0,0,0,0,0,0,0,0")
    assert "split input:" not in err
    ms = members_of(err)
    assert len(ms) == 8
    if form == "bgzf":
        assert any(m[4] == 0 and m[2] == m[1] for m in ms), ms
    else:
        sizes = [m[2] - m[1] for m in ms]
        assert max(sizes) - min(sizes) <= 1 and min(sizes) > 0, ms


def one_short_line(text: bytes) -> bytes:
    """the header and the first alignment line, with a SEQ of one base"""
    lines = text.splitlines(keepends=True)
    k = next(i for i, l in enumerate(lines) if not l.startswith(b"@"))
    f = lines[k].split(b"\t")
    f[5], f[9] = b"1M", b"A"
    return b"".join(lines[:k]) + b"\t".join(f)


def test_split_input_more_members_than_text_bytes(tmp_path):
    """Plain text of one short line for 64 members: most ranges are empty (one push of no bytes), the others hold a byte
    of the line each, and member 0 decodes it."""
    devices = ",".join(["0"] * 64)
    err = split_matches_one_device(tmp_path, with_names(tiny_case()), "sam", devices, oracle=False, edit=one_short_line)
    assert "split input:" not in err
    ms = members_of(err)
    assert len(ms) == 64
    assert sum(1 for m in ms if m[2] == m[1]) >= 8 and all(m[2] - m[1] <= 1 for m in ms), ms
    assert sum(m[4] for m in ms) == 0   # (no range holds a whole line: the stitch decodes it)


@pytest.mark.parametrize("form", FORMS)
def test_split_input_every_member_reads_its_share(tmp_path, form):
    w = with_names(make_workload(CONFIGS["config1"], seed=41, n_records=200_000))
    err = split_matches_one_device(tmp_path, w, form, "0,0,0,0", oracle=False)
    ms = members_of(err)
    assert len(ms) == 4
    sizes = [hi - lo for _, lo, hi, _, _ in ms]
    if form == "sam":   # (cut anywhere: equal to within a byte)
        assert max(sizes) - min(sizes) <= 1, ms
    else:               # (cut at block starts: as for BAM)
        total = ms[0][3]
        assert all(0.5 * total / 4 <= s <= 1.5 * total / 4 for s in sizes), ms


@pytest.mark.parametrize("form", FORMS)
def test_split_input_head_off_by_one_falls_back_to_member_0(tmp_path, form):
    err = split_matches_one_device(tmp_path, with_names(config1()), form, "0,0,0", env={"SLIMM_FORCE": "split_shift_guess"}, fallback=True)
    assert "split input:" in err and "reading the file through member 0" in err


@pytest.mark.parametrize("form", FORMS)
def test_one_device_takes_more_records_than_one_context(tmp_path, form):
    """SLIMM_FORCE record_cap: a context takes a third of the file's records; contexts of a group on the one device read a
    byte range each."""
    w = with_names(config1())
    one, _ = files_of(tmp_path, w, form, "one", [])
    n = len(w.records.read_key)
    got, err = files_of(tmp_path, w, form, "capped", ["--window-mb", "1"], env={"SLIMM_FORCE": f"record_cap={n // 3}"})
    assert got == one
    assert "reading the file by byte range" in err


@pytest.mark.parametrize("form", FORMS)
def test_split_input_q18_runs_apart_regroup_like_one_device(tmp_path, form):
    w = q18_apart_case()
    got, err = files_of(tmp_path, w, form, "split", ["--devices", "0,0,0,0", "--split-input"])
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=True, want_cov=True)
    check_outputs(str(tmp_path / "split"), STEM[form], o)
    assert "again as a file in no particular order" in err
    assert f"{Q18_APART_EXPECTED['matches']} matching reads" in err


@pytest.mark.parametrize("form", FORMS)
def test_split_input_q18_pairs_across_cuts(tmp_path, form):
    """Every read is an unflagged `p.1` followed by `p` with the first-mate flag: one run each (Q18), no regroup -- also
    where a cut lies between the two lines."""
    t = tiny_case()
    rng = random.Random(3)
    rows = []
    for i in range(6000):
        rows.append((f"p{i}.1", 0, rng.choice(t.ref_names[:4]), rng.randint(1, 800)))
        rows.append((f"p{i}", 0x41, rng.choice(t.ref_names[:4]), rng.randint(1, 800)))
    w = Workload(t.ref_names, t.ref_len, t.taxonomy, records_from_sam(rows, t.ref_names), avg_read_len=50, options=t.options,
                 name="q18-pairs")
    one, err1 = files_of(tmp_path, w, form, "one", [])
    got, err = files_of(tmp_path, w, form, "split", ["--devices", "0,0,0,0,0,0,0,0", "--split-input"])
    assert got == one
    assert "no particular order" not in err and "no particular order" not in err1
    assert "split input:" not in err
    assert len(members_of(err)) == 8 and "device decode on member 0" not in err


@pytest.mark.parametrize("form", FORMS)
def test_split_input_last_line_without_its_newline(tmp_path, form):
    """Only the file's last member ends such a line; the ranges that end inside the file end inside lines."""
    err = split_matches_one_device(tmp_path, with_names(config1()), form, "0,0,0,0", edit=lambda text: text[:-1])
    assert "split input:" not in err
    assert len(members_of(err)) == 4


def test_split_input_leaves_a_gzip_sam_on_todays_path(tmp_path):
    """One deflate stream cannot be cut: member 0 reads the file, and says why under SLIMM_TRACE=cli."""
    err = split_matches_one_device(tmp_path, with_names(config1()), "gzip", "0,0,0,0", fallback=True)
    assert "--split-input: a gzip stream is not cut by byte range" in err
    assert not members_of(err) and "split input:" not in err
