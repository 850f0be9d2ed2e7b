"""Corners of bzip2 blocks on the device (slimm_push_bzip2_sam_bytes, bzip2_decode.hip): blocks whose text repeats itself --
their inverse BWT has several cycles, and the text is the one through origPtr again and again -- give what
slimm_push_sam_bytes gives on the same text, in the API and in the command; block candidates injected inside real blocks
(SLIMM_FORCE bzip2_false_magics) are in fact decoded and dropped; a block longer than its stream's level allows is refused."""
import os
import re

import numpy as np
import pytest

from slimm_amd.profiler import Slimm
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_sam, write_sldb
from tests.cases import tiny_case
from tests.sam_bz2 import header_len, streams
from tests.test_cli_bzip2_sam_blocks import noisy_text, periodic_copy, too_long_for_level_1
from tests.test_cli_gpu import with_names
from tests.test_gpu_bam_decode import _named
from tests.test_gpu_compressed_sam import integers, outputs, run_cli

pytestmark = pytest.mark.gpu

REFUSED = "bzip2-compressed input is not supported unless it decodes"


def profile(w, push, grouped=False):
    s = Slimm.for_workload(w, device=0, grouped=grouped)
    s.set_reference_names(w.ref_names)
    n = push(s)
    s.get_profiles()
    out = integers(s)
    s.close()
    return n, out


@pytest.mark.parametrize("times", [2, 3])
@pytest.mark.parametrize("window", [0, 700])
def test_blocks_whose_text_repeats_itself_give_the_partials_of_the_text(tmp_path, times, window):
    w = _named(tiny_case())
    p = str(tmp_path / "t.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    plain, blob = periodic_copy(open(p, "rb").read(), times)
    skip = header_len(plain)
    want = profile(w, lambda s: s.push_sam_bytes(plain[skip:]))
    got = profile(w, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, window=window))
    assert want[0] == times * len(w.records)
    assert got == want


@pytest.mark.skipif(os.environ.get("SLIMM_EMU") == "1", reason="the command loads the GPU library")
def test_cli_reads_blocks_whose_text_repeats_itself(tmp_path):
    w = with_names(tiny_case())
    db = str(tmp_path / "db.sldb")
    write_sldb(db, w.taxonomy)
    p = str(tmp_path / "t.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    plain, blob = periodic_copy(open(p, "rb").read(), 2)
    d = str(tmp_path / "run") + "/"
    os.makedirs(d)
    open(d + "x.sam", "wb").write(plain)
    open(d + "x.sam.bz2", "wb").write(blob)
    base = ["-w", str(w.options.bin_width), "-ro", "-co"]
    plain_dir = d + "plain/"
    os.makedirs(plain_dir)
    run_cli(base + ["-o", plain_dir, db, d + "x.sam"])
    run_cli(base + [db, d + "x.sam.bz2"])   # (outputs next to the input, named after its whole name)
    assert outputs(d, "x.sam.bz2") == outputs(plain_dir, "x")


def false_magics(err: str) -> int:
    m = re.findall(r"\[push bzip2\] \d+ streams, \d+ blocks in \d+ batches, (\d+) false magics", err)
    assert m, err[-500:]
    return int(m[-1])


def test_false_magics_are_decoded_and_dropped(tmp_path, monkeypatch, capfd):
    w = _named(make_workload(CONFIGS["config1"], seed=31, n_records=3_000))
    p = str(tmp_path / "t.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(p, "rb").read()
    skip = header_len(text)
    blob = streams(text, chunk=len(text) // 4 + 1)
    monkeypatch.setenv("SLIMM_TRACE", "push")
    monkeypatch.delenv("SLIMM_FORCE", raising=False)
    capfd.readouterr()
    want = profile(w, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, window=70_000), grouped=True)
    assert false_magics(capfd.readouterr().err) == 0
    monkeypatch.setenv("SLIMM_FORCE", "bzip2_false_magics=997")
    got = profile(w, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, window=70_000), grouped=True)
    injected = false_magics(capfd.readouterr().err)
    assert injected >= len(blob) * 8 // 997 // 2   # (every 997 bits, and a few bits into every real block)
    assert got == want


def test_a_block_longer_than_its_level_allows_is_refused():
    w = _named(tiny_case())
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception) as e:
        s.push_bzip2_sam_bytes(too_long_for_level_1(noisy_text()), skip=2)
    s.close()
    assert f"{REFUSED}: block at byte 4: block longer than its stream's level allows" in str(e.value)
