"""`slimm -d --devices a,b,... --file-per-device`: the files of a directory side by side, one per listed slot.

The contract is the sequential run: every output file byte for byte what `-d --device 0` writes for the same directory, the
per-file blocks of the log whole and in list order, the closing total equal.  What one file hands to the files behind it
(bin width, min_reads, the two cached cut-offs: Q8) is carried through the first files, read in turn, until it is settled;
SLIMM_TRACE=cli says how many files that took (M) and which slot read which file.

The list order is the directory's `readdir` order.  The tests create the files empty, read the order with os.listdir and
then write the contents into the existing names, so that they decide which contents come first.
"""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import sam_header, write_bam, write_sam, write_sldb
from tests.cases import Q18_APART_EXPECTED, q18_apart_case
from tests.test_cli_gpu import CLI, check_outputs, with_names

pytestmark = pytest.mark.gpu

SIX = (0.0, 0.10, 0.25, 0.45, 0.60, 0.82, 1.0)   # (uneven: every file has its own record count)
COMMON = ["-ro", "-co", "-v"]
NO_HITS = "[WARNING] No mapped reads found in BAM file!"
AGAIN = "again as a file in no particular order"


@dataclasses.dataclass
class Part:
    """What one file of the directory holds: records (written as SAM or BAM, by the name's extension) or the bytes as given."""
    records: object = None
    read_len: int = 100
    raw: bytes = None


@pytest.fixture(scope="module")
def base():
    return with_names(make_workload(CONFIGS["config1"], seed=43))


def parts_of(w, cuts=SIX, read_lens=None):
    n = len(w.records)
    at = [int(round(c * n)) for c in cuts]
    return [Part(w.records.take(np.arange(at[k], at[k + 1])), read_lens[k] if read_lens else w.avg_read_len) for k in range(len(at) - 1)]


def unmapped(part):
    rec = part.records.take(np.arange(len(part.records)))
    rec.flag[:] = 4
    if rec.file_flag is not None:
        rec.file_flag[:] = 4
    return Part(rec, part.read_len)


def make_directory(d, w, parts, names=None):
    """The directory with one file per part; returns the file names in list order (parts[k] is in the k-th of them)."""
    d.mkdir()
    for nm in names or [f"s{k}.{'sam' if k % 2 == 0 else 'bam'}" for k in range(len(parts))]:
        (d / nm).touch()
    order = os.listdir(d)
    for nm, p in zip(order, parts):
        if p.raw is not None:
            with open(d / nm, "wb") as f:
                f.write(p.raw)
        else:
            (write_sam if nm.endswith(".sam") else write_bam)(str(d / nm), w.ref_names, w.ref_len, p.records, read_len=p.read_len)
    assert os.listdir(d) == order
    return order


def slimm(args, trace=False):
    env = dict(os.environ)
    env.pop("SLIMM_TRACE", None)
    if trace:
        env["SLIMM_TRACE"] = "cli"
    return subprocess.run([CLI] + args, capture_output=True, text=True, env=env)


HEAD = re.compile(r"^Reading (\d+) of (\d+) files \.\.\. \((.+)\)$")


def blocks_of(err):
    """([(k, name, lines)] of the per-file blocks in the order printed, the lines outside them); [trace] lines left out,
    the whole seconds of the timers made equal."""
    blocks, outside, cur = [], [], None
    for line in err.split("\n"):
        if line.startswith("[trace]"):
            continue
        line = re.sub(r"\d+ secs", "N secs", line)
        m = HEAD.match(line)
        if m:
            cur = (int(m.group(1)), m.group(3), [])
            blocks.append(cur)
            continue
        if line.startswith("*****"):
            cur = None
        (outside if cur is None else cur[2]).append(line)
    return blocks, outside


def files_in(out):
    return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


def total_line(outside):
    got = [l for l in outside if l.endswith("SAM/BAM alignment records are proccessed.")]
    assert len(got) == 1, outside
    return got[0]


def trace_of(err, n, slots):
    """(iv): M of the summary line, and {file index: slot} of the n per-file lines -- every file once, every slot below S."""
    m = re.findall(r"^\[trace\] file-per-device: (\d+) of (\d+) files read in turn before the carried values settled; "
                   r"(\d+) handed to (\d+) slots$", err, re.M)
    assert len(m) == 1, err[-3000:]
    M, N, rest, S = map(int, m[0])
    assert (N, rest, S) == (n, n - M, slots)
    per_file = re.findall(r"^\[trace\] file-per-device: file (\d+) \((.+)\) in slot (\d+) on device (\d+)$", err, re.M)
    assert sorted(int(k) for k, _, _, _ in per_file) == list(range(1, n + 1))
    assert all(int(j) < slots and int(dev) == 0 for _, _, j, dev in per_file)
    assert all(int(j) == 0 for k, _, j, _ in per_file if int(k) <= M)   # (read in turn: slot 0)
    return M, {int(k): (nm, int(j)) for k, nm, j, _ in per_file}


def stem(name):
    return name[:-4]


def run_both(tmp_path, db, inp, args, devices, directory=True):
    """The sequential run and the --file-per-device run (SLIMM_TRACE=cli) of one input: {tag: (out, CompletedProcess)}"""
    runs = {}
    for tag, extra in (("seq", ["--device", "0"]), ("fpd", ["--devices", devices, "--file-per-device"])):
        out = str(tmp_path / tag) + "/"
        os.makedirs(out)
        runs[tag] = (out, slimm((["-d"] if directory else []) + extra + args + ["-o", out, db, inp], trace=tag == "fpd"))
    return runs


def check_directory(tmp_path, w, parts, devices, args, M, options, names=None):
    """Points (i) to (v) for one directory; returns the blocks of the --file-per-device run."""
    order = make_directory(tmp_path / "in", w, parts, names)
    n, slots = len(parts), devices.count(",") + 1
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    runs = run_both(tmp_path, db, str(tmp_path / "in"), args + COMMON, devices)
    for out, r in runs.values():
        assert r.returncode == 0, r.stderr[-3000:]
    (seq_out, seq), (out, fpd) = runs["seq"], runs["fpd"]
    # (i) the sequential run's files, byte for byte
    assert files_in(out) == files_in(seq_out)
    # (iii) the blocks in list order, each whole: line for line the sequential run's block of that file
    blocks, outside = blocks_of(fpd.stderr)
    seq_blocks, seq_outside = blocks_of(seq.stderr)
    assert [(k, nm) for k, nm, _ in blocks] == [(k + 1, nm) for k, nm in enumerate(order)]
    assert blocks == seq_blocks
    # (ii) one Oracle object over the files in the order of the printed blocks
    orc = Oracle(w.taxonomy, options)
    with_hits = 0
    for k, nm, lines in blocks:
        p = parts[k - 1]
        counted = [l for l in lines if l.endswith(" records processed.")]
        o = None if p.raw is not None else orc.run(w.ref_names, w.ref_len, p.records, p.read_len, want_raw=True, want_cov=True)
        if o is None or o.no_hits:
            assert not counted and not os.path.exists(os.path.join(out, stem(nm) + "_profile.tsv"))
            assert lines.count(NO_HITS) == (0 if o is None else 1)
            continue
        with_hits += 1
        check_outputs(out, stem(nm), o)
        assert counted == [f"  {o.scalars['hits']} records processed."], (nm, counted)   # (iii): file k's count, once
        assert sum(l.startswith("[Done!] File took") for l in lines) == 1
    assert len(files_in(out)) == 5 * with_hits
    # (iv) the two trace lines
    got_M, where = trace_of(fpd.stderr, n, slots)
    assert [where[k + 1][0] for k in range(n)] == order
    if M is not None:
        assert got_M == M
    # (v) the closing total
    assert total_line(outside) == total_line(seq_outside)
    return blocks


def test_six_files_two_slots_on_one_device(tmp_path, base):
    parts = parts_of(base)
    blocks = check_directory(tmp_path, base, parts, "0,0", ["-w", "100"], 1, base.options)
    counts = [l for _, _, lines in blocks for l in lines if l.endswith(" records processed.")]
    assert len(set(counts)) == 6   # (a count in the wrong block would show)


def test_more_slots_than_files(tmp_path, base):
    check_directory(tmp_path, base, parts_of(base, (0.0, 0.4, 1.0)), "0,0,0", ["-w", "100"], 1, base.options)


def test_first_file_without_hits_settles_nothing(tmp_path, base):
    """min_reads and the cut-offs come from the first file WITH hits: the second one here, so two files are read in turn."""
    parts = parts_of(base)
    parts[0] = unmapped(parts[0])
    check_directory(tmp_path, base, parts, "0,0", ["-w", "100"], 2, base.options)


def test_everything_given_every_file_is_handed_out(tmp_path, base):
    options = dataclasses.replace(base.options, min_reads=5, cov_cut_off=1.0)
    check_directory(tmp_path, base, parts_of(base), "0,0", ["-w", "100", "-mr", "5", "-cc", "1.0"], 0, options)


def test_bin_width_comes_from_the_first_file_alone(tmp_path, base):
    lens = [80, 100, 60, 90, 70, 50]
    options = dataclasses.replace(base.options, bin_width=0)
    check_directory(tmp_path, base, parts_of(base, read_lens=lens), "0,0", [], 1, options)


def test_no_file_has_hits_every_file_in_turn(tmp_path, base):
    parts = [unmapped(p) for p in parts_of(base, (0.0, 0.01, 0.03, 0.06))]
    blocks = check_directory(tmp_path, base, parts, "0,0", ["-w", "100"], 3, base.options)
    assert [lines.count(NO_HITS) for _, _, lines in blocks] == [1, 1, 1]


def test_each_file_is_read_again_in_any_order_inside_its_block(tmp_path):
    w = q18_apart_case()
    names = ["apart.sam", "again.bam", "third.sam"]
    blocks = check_directory(tmp_path, w, [Part(w.records, w.avg_read_len)] * 3, "0,0", ["-w", "100"], None, w.options, names)
    for _, _, lines in blocks:
        assert sum(AGAIN in l for l in lines) == 1
        assert lines.count(f"    {Q18_APART_EXPECTED['matches']} matching reads") == 1
        assert lines.count("  54 records processed.") == 1


def test_a_file_that_open_refuses_is_skipped(tmp_path, base):
    parts = parts_of(base)
    parts[2] = Part(raw=b"\xfd7zXZ\x00" + bytes(range(256)) * 8)
    blocks = check_directory(tmp_path, base, parts, "0,0", ["-w", "100"], 1, base.options)
    assert sum("xz-compressed input is not supported" in l for l in blocks[2][2]) == 1


def test_a_failing_file_ends_the_run_with_its_block_the_last(tmp_path, base):
    """A SAM file whose records carry no sequence ends the sequential run with status 1, here too: the blocks of the files
    before it, then its own with the message, and no closing lines."""
    parts = parts_of(base)
    text = sam_header(base.ref_names, base.ref_len) + "".join(
        f"q{i}\t0\t{base.ref_names[0]}\t{10 + i}\t255\t*\t*\t0\t0\t*\t*\n" for i in range(20))
    parts[3] = Part(raw=text.encode())
    order = make_directory(tmp_path / "in", base, parts)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, base.taxonomy)
    runs = run_both(tmp_path, db, str(tmp_path / "in"), ["-w", "100"] + COMMON, "0,0")
    (seq_out, seq), (out, fpd) = runs["seq"], runs["fpd"]
    assert seq.returncode == 1 and fpd.returncode == 1
    blocks, outside = blocks_of(fpd.stderr)
    seq_blocks, _ = blocks_of(seq.stderr)
    assert [(k, nm) for k, nm, _ in blocks] == [(k + 1, nm) for k, nm in enumerate(order[:4])]
    assert blocks == seq_blocks
    assert sum("[ERROR] no record with a sequence" in l for l in blocks[-1][2]) == 1
    assert not any("alignment records are proccessed" in l for l in outside)
    # the files before the failing one are the sequential run's (those behind it may or may not have been started)
    mine, theirs = files_in(out), files_in(seq_out)
    assert len(theirs) == 15 and all(mine[f] == theirs[f] for f in theirs)
    assert not os.path.exists(os.path.join(out, stem(order[3]) + "_profile.tsv"))


def test_one_file_without_directory_runs_in_slot_0(tmp_path, base):
    db = str(tmp_path / "db.sldb")
    write_sldb(db, base.taxonomy)
    inp = str(tmp_path / "sample.bam")
    write_bam(inp, base.ref_names, base.ref_len, base.records, read_len=base.avg_read_len)
    runs = run_both(tmp_path, db, inp, ["-w", "100"] + COMMON, "0,0", directory=False)
    for out, r in runs.values():
        assert r.returncode == 0, r.stderr[-3000:]
    (seq_out, seq), (out, fpd) = runs["seq"], runs["fpd"]
    assert files_in(out) == files_in(seq_out) and len(files_in(out)) == 5
    o = Oracle(base.taxonomy, base.options).run(base.ref_names, base.ref_len, base.records, base.avg_read_len, want_raw=True, want_cov=True)
    check_outputs(out, "sample", o)
    blocks, outside = blocks_of(fpd.stderr)
    seq_blocks, seq_outside = blocks_of(seq.stderr)
    assert blocks == seq_blocks and len(blocks) == 1
    assert trace_of(fpd.stderr, 1, 2) == (1, {1: ("sample.bam", 0)})
    assert total_line(outside) == total_line(seq_outside)
