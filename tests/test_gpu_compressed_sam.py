"""Compressed SAM on a real MI355X: slimm_push_bgzf_sam_blocks (BGZF blocks of SAM text inflated, found and decoded on the
device) against slimm_push_sam_bytes on the same text, and the `slimm` command on gzip and BGZF copies of a SAM file against
the plain file's run and the CPU oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle, run_workload
from slimm_amd.profiler import Slimm
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_sam, write_sldb
from tests.cases import q18_apart_case, tiny_case
from tests.helpers import assert_matches_oracle
from tests.sam_gz import bgzf, gzip_members, header_len
from tests.test_gpu_bam_decode import _named
from tests.test_cli_gpu import check_outputs, with_names

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)


def sam_text(tmp_path, w, tail_newline=True) -> bytes:
    p = str(tmp_path / "abi.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(p, "rb").read()
    return text if tail_newline else text[:-1]


def integers(s):
    st = s.stats()
    rc = s.ref_columns()
    return ({k: v for k, v in st.items() if isinstance(v, (int, np.integer))},
            {k: np.asarray(v).tolist() for k, v in rc.items() if np.asarray(v).dtype.kind in "iub"},
            [s.bins(k).tolist() for k in range(3)], s.taxon_counts(0), s.taxon_counts(1), s.children_pairs(1))


def profile_of(w, grouped, push):
    s = Slimm.for_workload(w, device=0, grouped=grouped)
    s.set_reference_names(w.ref_names)
    n = push(s)
    assert n == len(w.records)
    s.get_profiles()
    out = integers(s)
    return s, out


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("window,host_every,seed", [(0, 0, 1), (60_000, 0, 2), (8_000, 2, 3), (200_000, 3, 4), (1 << 20, 1, 5)])
def test_bgzf_sam_blocks_give_the_partials_of_the_text(tmp_path, grouped, window, host_every, seed):
    """Windows cut at block boundaries with the header skipped in the first one; every host_every-th window inflated by the
    host and pushed as text (the two forms alternate); blocks cut inside lines."""
    w = _named(make_workload(CONFIGS["config1"], seed=31, shuffled=not grouped))
    text = sam_text(tmp_path, w)
    skip = header_len(text)
    blob = bgzf(text, seed=seed, lo=500, hi=65_000)
    o = run_workload(w, use_qnames=True)
    s1, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:], window=window))
    s2, got = profile_of(w, grouped, lambda s: s.push_bgzf_sam_blocks(blob, skip=skip, window=window, host_every=host_every))
    assert got == want
    assert_matches_oracle(s2, o)
    s1.close()
    s2.close()


@pytest.mark.parametrize("host_every", [0, 2])
@pytest.mark.parametrize("window", [0, 30_000])
def test_last_line_without_newline_inflated_on_the_device(tmp_path, host_every, window):
    """The device inflated the text's end, and the last line has no newline: the device ends it (the host never sees those
    bytes).  Also when the last push carries no bytes (an end-of-file block only)."""
    w = _named(make_workload(CONFIGS["config1"], seed=33))
    text = sam_text(tmp_path, w, tail_newline=False)
    skip = header_len(text)
    o = run_workload(w, use_qnames=True)
    for eof in (True, False):
        blob = bgzf(text, seed=9, lo=3000, hi=20_000, eof=eof)
        s, _ = profile_of(w, True, lambda s: s.push_bgzf_sam_blocks(blob, skip=skip, window=window, host_every=host_every))
        assert_matches_oracle(s, o)
        s.close()
    # every byte inflated on the device in one window, the last push empty
    blob = bgzf(text, seed=9, lo=3000, hi=20_000, eof=False)
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    got, buf = C.c_uint64(), np.frombuffer(blob, dtype=np.uint8).copy()
    s._check(s.L.slimm_push_bgzf_sam_blocks(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 0, C.byref(got)))
    n = got.value
    s._check(s.L.slimm_push_bgzf_sam_blocks(s.ctx, None, 0, 0, 1, C.byref(got)))
    assert n + got.value == len(w.records)
    s.get_profiles()
    assert_matches_oracle(s, o)
    s.close()


def test_corrupt_block_and_mixing_with_bam_are_errors(tmp_path):
    w = _named(tiny_case())
    text = sam_text(tmp_path, w)
    skip = header_len(text)
    blob = bytearray(bgzf(text, seed=1, lo=50, hi=120))
    p = 0
    for _ in range(3):
        p += (blob[p + 16] | (blob[p + 17] << 8)) + 1
    blob[p + 20] ^= 0xff   # inside the third block's deflate data
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception) as e:
        s.push_bgzf_sam_blocks(bytes(blob), skip=skip)
    assert "corrupt BGZF block" in str(e.value)
    s.close()
    # a BGZF SAM push behind BAM bytes of the same file
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    got = C.c_uint64()
    filler = np.zeros(64, dtype=np.uint8)
    assert s.L.slimm_push_bam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 0, 0, C.byref(got)) == SLIMM_OK
    blob = np.frombuffer(bgzf(text, seed=1), dtype=np.uint8).copy()
    rc = s.L.slimm_push_bgzf_sam_blocks(s.ctx, blob.ctypes.data_as(C.c_void_p), blob.size, skip, 1, C.byref(got))
    assert rc == SLIMM_E_INVALID
    s.close()


# ---- the command ---------------------------------------------------------------------------------------------------------
MODES = {
    "device": [],
    "host_decode": ["--host-decode"],
    "any_order": ["--any-order"],
    "devices": ["--devices", "0,0"],
    "inflate1": ["--device-inflate", "1", "--window-mb", "1"],
    "inflate2": ["--device-inflate", "2", "--window-mb", "1"],
}


def run_cli(args):
    r = subprocess.run([CLI] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def outputs(d, stem):
    return {sfx: open(os.path.join(d, stem + sfx + ".tsv"), "rb").read()
            for sfx in ("_profile", "_raw", "_coverage", "_uniq_coverage", "_uniq_coverage2")}


def cli_case(tmp_path, w, modes, tail_newline=True, seed=0):
    w = with_names(w)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(sam, "rb").read()
    if not tail_newline:
        open(sam, "wb").write(text[:-1])
        text = text[:-1]
    copies = {"bgzf": bgzf(text, seed=seed, lo=20_000, hi=65_000), "gzip": gzip_members(text, 2)}
    o = Oracle(w.taxonomy, w.options).run(w.ref_names, w.ref_len, w.records, w.avg_read_len, want_raw=True, want_cov=True)
    for mode in modes:
        base = ["-w", str(w.options.bin_width), "-ro", "-co"] + MODES[mode]
        plain_dir = str(tmp_path / f"plain_{mode}") + "/"
        os.makedirs(plain_dir)
        run_cli(base + ["-o", plain_dir, db, sam])
        want = outputs(plain_dir, "x")
        check_outputs(plain_dir, "x", o)
        for kind, blob in copies.items():
            d = str(tmp_path / f"{kind}_{mode}")
            os.makedirs(d)
            inp = os.path.join(d, "x.sam.gz")
            open(inp, "wb").write(blob)
            run_cli(base + [db, inp])   # (outputs next to the input: x.sam.gz keeps its whole name, like the reference)
            assert outputs(d, "x.sam.gz") == want, (kind, mode)


@pytest.mark.parametrize("case", ["tiny", "q18_apart", "config1"])
def test_cli_compressed_sam_writes_the_files_of_the_plain_sam(tmp_path, case):
    w = {"tiny": tiny_case, "q18_apart": q18_apart_case, "config1": lambda: make_workload(CONFIGS["config1"], seed=41)}[case]()
    cli_case(tmp_path, w, sorted(MODES))


@pytest.mark.parametrize("tail_newline", [True, False])
def test_cli_compressed_sam_lines_straddle_blocks_and_windows(tmp_path, tail_newline):
    """Windows of 1 MB, a file of ~30 MB of text: lines straddle blocks and windows, windows inflated on the host and on the
    device alternate, and the last line has its newline or not."""
    w = make_workload(CONFIGS["config2"], seed=45, n_records=200_000)
    cli_case(tmp_path, w, ["inflate1", "inflate2", "any_order"], tail_newline=tail_newline, seed=3)


def test_cli_10m_record_bgzf_sam_has_the_profile_of_the_plain_sam(tmp_path):
    w = with_names(make_workload(CONFIGS["config3"], seed=47, n_records=10_000_000))
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=100)   # (1.3 GB of text; -w below fixes the bin width)
    text = open(sam, "rb").read()
    d = str(tmp_path / "gz")
    os.makedirs(d)
    inp = os.path.join(d, "x.sam.gz")
    open(inp, "wb").write(bgzf(text, seed=5, lo=65_000, hi=65_280))
    del text
    run_cli(["-w", "1000", "-o", str(tmp_path) + "/", db, sam])
    run_cli(["-w", "1000", db, inp])
    assert open(os.path.join(d, "x.sam.gz_profile.tsv"), "rb").read() == open(str(tmp_path / "x_profile.tsv"), "rb").read()
