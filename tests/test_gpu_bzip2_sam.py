"""bzip2-compressed SAM on a real MI355X: slimm_push_bzip2_sam_bytes (the file's bytes, cut anywhere; blocks found, decoded
and checked on the device, the text found and decoded as SAM) against slimm_push_sam_bytes on the same text and the CPU
oracle, and the `slimm` command on bzip2 copies of a SAM file against the plain file's run and the oracle."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from oracle.binding import Oracle, run_workload
from slimm_amd.profiler import Slimm
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_sam, write_sldb
from tests.cases import q18_apart_case, tiny_case
from tests.helpers import assert_matches_oracle
from tests.sam_bz2 import EOS_MAGIC, flip_bit, header_len, magics, one_stream, set_bits, streams
from tests.test_cli_gpu import check_outputs, with_names
from tests.test_gpu_bam_decode import _named
from tests.test_gpu_compressed_sam import outputs, profile_of, run_cli, sam_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)
REFUSED = "bzip2-compressed input is not supported unless it decodes"
EMU = os.environ.get("SLIMM_EMU") == "1"


def forced(monkeypatch, value):
    if value:
        monkeypatch.setenv("SLIMM_FORCE", value)
    else:
        monkeypatch.delenv("SLIMM_FORCE", raising=False)


def random_cuts(n, seed, lo, hi):
    rng, p, out = random.Random(seed), 0, []
    while True:
        p += rng.randint(lo, hi)
        if p >= n:
            return out
        out.append(p)


def workload(grouped, small=False):
    w = make_workload(CONFIGS["config1"], seed=31, shuffled=not grouped, n_records=3_000 if small or EMU else None)
    return _named(w)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind", ["level1", "level9", "streams"])
@pytest.mark.parametrize("cut,force", [("one", ""), ("random", "bzip2_round=1"), ("60k", "bzip2_round=100000"), ("1m", "")])
def test_bzip2_sam_bytes_give_the_partials_of_the_text(tmp_path, monkeypatch, grouped, kind, cut, force):
    """The file's bytes pushed whole, cut at random offsets (inside blocks and magics; with bzip2_round=1 every push is
    decoded as far as it goes and a block's bytes wait for the next push), in 60 kB or 1 MB windows; one stream of level 1
    or 9, or streams of different levels back to back with an empty one among them."""
    w = workload(grouped)
    text = sam_text(tmp_path, w)
    skip = header_len(text)
    blob = {"level1": one_stream(text, 1), "level9": one_stream(text, 9), "streams": streams(text, chunk=len(text) // 5 + 1)}[kind]
    cuts = {"one": [], "random": random_cuts(len(blob), 7, 1, 9_000), "60k": list(range(60_000, len(blob), 60_000)),
            "1m": list(range(1 << 20, len(blob), 1 << 20))}[cut]
    o = run_workload(w, use_qnames=True)
    s1, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:]))
    forced(monkeypatch, force)
    s2, got = profile_of(w, grouped, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, cuts=cuts))
    assert got == want
    assert_matches_oracle(s2, o)
    s1.close()
    s2.close()


@pytest.mark.parametrize("force", ["", "bzip2_round=1"])
def test_last_line_without_newline(tmp_path, monkeypatch, force):
    """The text's last line has no newline: it is a line all the same -- also when the last push carries no byte."""
    w = workload(True)
    text = sam_text(tmp_path, w, tail_newline=False)
    skip = header_len(text)
    o = run_workload(w, use_qnames=True)
    forced(monkeypatch, force)
    for empty_last in (False, True):
        for blob in (one_stream(text, 9), streams(text, chunk=len(text) // 3 + 1, empty_at=-1)):
            s, _ = profile_of(w, True, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, window=50_000, empty_last=empty_last))
            assert_matches_oracle(s, o)
            s.close()


def test_false_magics_inside_blocks_change_nothing(tmp_path, monkeypatch):
    """SLIMM_FORCE bzip2_false_magics: block candidates a few bits into every real block and every 997 bits are decoded and
    dropped by the chain; every output is that of the run without them."""
    w = workload(True)
    text = sam_text(tmp_path, w)
    skip = header_len(text)
    blob = streams(text, chunk=len(text) // 4 + 1)
    s1, want = profile_of(w, True, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, window=70_000))
    forced(monkeypatch, "bzip2_false_magics=997")
    s2, got = profile_of(w, True, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, window=70_000))
    assert got == want
    s1.close()
    s2.close()


def push_error(w, blob, skip):
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception) as e:
        s.push_bzip2_sam_bytes(blob, skip=skip, window=40_000)
    s.close()
    return str(e.value)


def test_damage_is_an_error_and_bzip2_does_not_mix_with_bam(tmp_path):
    w = workload(True, small=True)
    text = sam_text(tmp_path, w)
    skip = header_len(text)
    blob = one_stream(text, 9)
    first, eos = magics(blob)[0], magics(blob, EOS_MAGIC)[-1]
    cases = {
        "huffman_bit": (flip_bit(blob, first + 48 + 32 + 1 + 24 + 16 + 1500), "block at byte"),
        "block_crc": (flip_bit(blob, first + 48 + 9), "block CRC mismatch"),
        "combined_crc": (flip_bit(blob, eos + 48 + 1), "combined CRC mismatch"),
        "orig_ptr": (set_bits(blob, first + 48 + 32 + 1, 24, 0xffffff), "origPtr out of range"),
        "randomised": (set_bits(blob, first + 48 + 32, 1, 1), "randomised block"),
        "truncated": (blob[:len(blob) // 2], "truncated"),
        "trailing": (blob + b"\x00junk", "bytes after the last end-of-stream marker"),
    }
    for name, (data, word) in cases.items():
        msg = push_error(w, data, skip)
        assert REFUSED in msg and word in msg, (name, msg)
    # bzip2 bytes behind BAM bytes of the same file, and BAM bytes behind bzip2 bytes
    got = C.c_uint64()
    filler = np.zeros(64, dtype=np.uint8)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_bam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 0, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_bzip2_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_bzip2_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_sam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 10, 1, C.byref(got)) == SLIMM_E_INVALID
    s.close()


# ---- the command ---------------------------------------------------------------------------------------------------------
MODES = {
    "device": [],
    "host_decode": ["--host-decode"],
    "any_order": ["--any-order"],
    "devices": ["--devices", "0,0"],
    "window1": ["--window-mb", "1"],
}


def cli_case(tmp_path, w, modes, tail_newline=True):
    w = with_names(w)
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(sam, "rb").read()
    if not tail_newline:
        open(sam, "wb").write(text[:-1])
        text = text[:-1]
    copies = {"level9": one_stream(text, 9), "streams": streams(text, chunk=400_000, workers=4)}
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
            inp = os.path.join(d, "x.sam.bz2")
            open(inp, "wb").write(blob)
            run_cli(base + [db, inp])   # (outputs next to the input: x.sam.bz2 keeps its whole name, like x.sam.gz)
            assert outputs(d, "x.sam.bz2") == want, (kind, mode)


@pytest.mark.parametrize("case", ["tiny", "q18_apart", "config1"])
def test_cli_bzip2_sam_writes_the_files_of_the_plain_sam(tmp_path, case):
    w = {"tiny": tiny_case, "q18_apart": q18_apart_case, "config1": lambda: make_workload(CONFIGS["config1"], seed=41)}[case]()
    cli_case(tmp_path, w, sorted(MODES))


@pytest.mark.parametrize("tail_newline", [True, False])
def test_cli_bzip2_sam_lines_straddle_blocks_and_windows(tmp_path, tail_newline):
    w = make_workload(CONFIGS["config2"], seed=45, n_records=200_000)
    cli_case(tmp_path, w, ["window1", "any_order"], tail_newline=tail_newline)


def test_cli_2m_record_bzip2_sam_has_the_profile_of_the_plain_sam(tmp_path):
    w = with_names(make_workload(CONFIGS["config3"], seed=47, n_records=2_000_000))
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    sam = str(tmp_path / "x.sam")
    write_sam(sam, w.ref_names, w.ref_len, w.records, read_len=100)
    text = open(sam, "rb").read()
    d = str(tmp_path / "bz")
    os.makedirs(d)
    inp = os.path.join(d, "x.sam.bz2")
    open(inp, "wb").write(streams(text, chunk=8 << 20, levels=(9,), empty_at=-1, workers=16))
    del text
    run_cli(["-w", "1000", "-o", str(tmp_path) + "/", db, sam])
    run_cli(["-w", "1000", db, inp])
    assert open(os.path.join(d, "x.sam.bz2_profile.tsv"), "rb").read() == open(str(tmp_path / "x_profile.tsv"), "rb").read()
