"""The record filter in the host reader (AlignmentFile::set_filter, host/alignment_file.cpp), through `slimm --dump-records`
with -q / --require-flags / --exclude-flags / --min-aligned / --min-identity: the flags handed on (0x4 on a dropped record)
and the counts on stderr against the Python restatement of the predicate (tests/record_filter_ref.py), on a SAM and on a
BAM file of a few thousand records with the edge records placed by hand.  No GPU is touched."""
import os
import subprocess

import pytest

from tests import record_filter_inputs as I
from tests import record_filter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")

M100 = [(100, "M")]
EDGES = [   # (what, Attr): records 0 .. of the file, all with flag 0x2 on a reference
    ("MAPQ 255 is a number", I.Attr(255, M100, [("NM", "i", 0)])),
    ("MAPQ 9", I.Attr(9, M100, [("NM", "i", 0)])),
    ("CIGAR *", I.Attr(60, None, [("NM", "i", 0)])),
    ("only S and H", I.Attr(60, [(10, "H"), (100, "S")], [("NM", "i", 0)])),
    ("I and D: 104 of 110 columns", I.Attr(60, [(40, "M"), (10, "I"), (40, "M"), (10, "D"), (10, "M")], [("NM", "i", 6)])),
    ("I and D: 105 of 110 columns", I.Attr(60, [(40, "M"), (10, "I"), (40, "M"), (10, "D"), (10, "M")], [("NM", "i", 5)])),
    ("exactly 950 per mille", I.Attr(60, M100, [("NM", "C", 5)])),
    ("one below 950 per mille", I.Attr(60, M100, [("NM", "C", 6)])),
    ("49 aligned bases", I.Attr(60, [(51, "S"), (49, "=")], [("NM", "c", 0)])),
    ("50 aligned bases", I.Attr(60, [(50, "S"), (50, "X")], [("NM", "c", 0)])),
] + [("NM as " + t, I.Attr(60, M100, [("AS", "i", 77), ("NM", t, 3)])) for t in "cCsSiI"] + [
    ("NM behind a Z tag", I.Attr(60, M100, [("MD", "Z", "50A49"), ("NM", "s", 7)])),
    ("NM behind an H tag", I.Attr(60, M100, [("XH", "H", "1AE301"), ("NM", "S", 7)])),
    ("NM behind a B:i tag", I.Attr(60, M100, [("XB", "B", ("i", [1, -2, 3])), ("NM", "I", 2)])),
    ("NM behind A and f tags", I.Attr(60, M100, [("XT", "A", "U"), ("XF", "f", 0.5), ("NM", "c", 2)])),
    ("NM absent", I.Attr(60, M100, [("MD", "Z", "100")])),
    ("NM > columns", I.Attr(60, M100, [("NM", "C", 120)])),
]
LAST = I.Attr(60, M100, [("MD", "Z", "100"), ("NM", "i", 1)])   # the file's last line: NM is its last field, no newline behind it


def cli_args(f):
    a = []
    if f["min_mapq"]:
        a += ["-q", str(f["min_mapq"])]
    if f["require_flags"]:
        a += ["--require-flags", str(f["require_flags"])]
    if f["exclude_flags"]:
        a += ["--exclude-flags", hex(f["exclude_flags"])]
    if f["min_aligned"]:
        a += ["--min-aligned", str(f["min_aligned"])]
    if f["min_identity_permille"]:
        a += ["--min-identity", "%.3f" % (f["min_identity_permille"] / 1000.0)]
    return a


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rf_host")
    w, attrs, lost = I.workload_and_attrs(grouped=True)
    r = w.records
    for k in list(range(len(EDGES))) + [len(r) - 1]:
        attrs[k] = EDGES[k][1] if k < len(EDGES) else LAST
        r.flag[k] = 0x2
        if int(r.ref_id[k]) in (-1, lost):   # (on a reference, and not on the one that is to lose all its reads)
            r.ref_id[k] = (lost + 1) % len(w.ref_names)
            r.begin_pos[k] = 0
    lines = I.sam_lines(w, attrs, tmp)
    bodies = I.bam_bodies(w, attrs)
    sam, bam = str(tmp / "x.sam"), str(tmp / "x.bam")
    open(sam, "wb").write(I.sam_file_text(w, lines, tail_newline=False))
    I.bam_file(bam, w, bodies)
    verdicts = {name: ([R.judge_sam(f, ln) for ln in lines], [R.judge_bam(f, b) for b in bodies]) for name, f in I.FILTERS.items()}
    return w, sam, bam, verdicts


def dump(path, args):
    r = subprocess.run([CLI, "--dump-records", *args, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    recs = [ln.split("\t") for ln in r.stdout.split("\n")[1:] if ln and not ln.startswith("@\t")]
    return recs, r.stderr


def test_the_inputs_are_what_the_tests_need(files):
    w, _sam, _bam, verdicts = files
    for name, (vs, vb) in verdicts.items():
        assert vs == vb, name   # (the two files hold the same records: one verdict each)
    I.input_conditions(w, {k: v[0] for k, v in verdicts.items()})
    v = verdicts["all"][0]
    want = {"MAPQ 255 is a number": R.PASS, "MAPQ 9": R.MAPQ, "CIGAR *": R.ALIGNED, "only S and H": R.ALIGNED,
            "I and D: 104 of 110 columns": R.IDENTITY, "I and D: 105 of 110 columns": R.PASS, "exactly 950 per mille": R.PASS,
            "one below 950 per mille": R.IDENTITY, "49 aligned bases": R.ALIGNED, "50 aligned bases": R.PASS, "NM behind a Z tag": R.IDENTITY,
            "NM behind an H tag": R.IDENTITY, "NM behind a B:i tag": R.PASS, "NM behind A and f tags": R.PASS, "NM absent": R.NO_NM,
            "NM > columns": R.IDENTITY}
    for k, (what, _a) in enumerate(EDGES):
        assert v[k] == want.get(what, R.PASS), what
    assert v[-1] == R.PASS
    vi = verdicts["identity"][0]
    assert vi[2] == R.IDENTITY and vi[3] == R.IDENTITY   # ("*" and S/H only: no columns, with an NM)


@pytest.mark.parametrize("fmt", ["sam", "bam"])
@pytest.mark.parametrize("name", list(I.FILTERS))
def test_dump_records_marks_and_counts_as_the_restatement(files, fmt, name):
    w, sam, bam, verdicts = files
    v = verdicts[name][0 if fmt == "sam" else 1]
    recs, err = dump(sam if fmt == "sam" else bam, cli_args(I.FILTERS[name]))
    assert len(recs) == len(w.records)
    want = [int(fl) | (4 if R.dropped(x) else 0) for fl, x in zip(w.records.flag.tolist(), v)]
    got = [int(r[1]) for r in recs]
    bad = [k for k in range(len(want)) if want[k] != got[k]]
    assert not bad, (bad[:10], [(want[k], got[k]) for k in bad[:10]])
    assert "#" + R.stats_line(R.count(v)) in err.split("\n")
    if name == "all":
        c = R.count(v)
        assert c["no_nm"] > 0 and all(c[k] > 0 for k in R.STATS)


@pytest.mark.parametrize("fmt", ["sam", "bam"])
def test_without_an_option_nothing_is_marked_and_no_line_is_printed(files, fmt):
    w, sam, bam, _ = files
    recs, err = dump(sam if fmt == "sam" else bam, [])
    assert [int(r[1]) for r in recs] == w.records.flag.tolist()
    assert "record filter" not in err
