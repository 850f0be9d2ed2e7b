"""The host's plans for a SAM file split by byte range (host only): slimm_host_text_ranges cuts plain text evenly and
anywhere behind the header -- the device finds the line starts --, and slimm_host_bgzf_ranges, given the header's inflated
length, makes no cut in front of the BGZF block that holds the first alignment line."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from slimm_amd import capi
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_sam
from tests.sam_gz import bgzf, header_len
from tests.test_split_ranges import block_starts


@pytest.fixture(scope="module")
def sam(tmp_path_factory):
    w = make_workload(CONFIGS["config1"], seed=41)
    p = str(tmp_path_factory.mktemp("sam") / "sample.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    return p, open(p, "rb").read()


def text_ranges(path, n, skip):
    out = (C.c_uint64 * (n + 1))()
    assert capi.lib().slimm_host_text_ranges(path.encode(), skip, n, out) == capi.OK
    return list(out)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 64])
def test_text_ranges_cover_the_alignment_lines_evenly(sam, n):
    path, text = sam
    skip = header_len(text)
    offs = text_ranges(path, n, skip)
    assert offs[0] == skip and offs[n] == len(text)
    assert all(a <= b for a, b in zip(offs, offs[1:]))
    sizes = np.diff(np.array(offs, dtype=np.int64))
    assert sizes.max() - sizes.min() <= 1


def test_more_ranges_than_bytes_gives_empty_ranges(tmp_path):
    p = str(tmp_path / "short.sam")
    open(p, "wb").write(b"@HD\tVN:1.6\nabc\n")
    offs = text_ranges(p, 16, 11)
    assert offs[0] == 11 and offs[16] == 15
    assert all(a <= b for a, b in zip(offs, offs[1:]))
    assert sum(1 for a, b in zip(offs, offs[1:]) if a == b) == 12
    assert text_ranges(p, 4, 15) == [15] * 5   # (a header only: every range is empty)


def test_not_a_file_or_a_skip_beyond_it(sam, tmp_path):
    path, text = sam
    out = (C.c_uint64 * 3)()
    L = capi.lib()
    assert L.slimm_host_text_ranges(str(tmp_path / "missing.sam").encode(), 0, 2, out) == capi.E_INVALID
    assert L.slimm_host_text_ranges(str(tmp_path).encode(), 0, 2, out) == capi.E_INVALID   # (a directory)
    assert L.slimm_host_text_ranges(path.encode(), len(text) + 1, 2, out) == capi.E_INVALID
    assert L.slimm_host_text_ranges(path.encode(), 0, 0, out) == capi.E_INVALID


def test_bgzf_sam_ranges_do_not_cut_in_front_of_the_first_alignment_line(sam, tmp_path):
    path, text = sam
    skip = header_len(text)
    blob = bgzf(text, seed=4, lo=200, hi=900)
    p = str(tmp_path / "sample.sam.gz")
    open(p, "wb").write(blob)
    # the block that holds inflated byte `skip`: the first alignment line starts in it
    before, holder = 0, None
    starts = block_starts(blob)
    for s in starts:
        isize = struct.unpack_from("<I", blob, s + struct.unpack_from("<H", blob, s + 16)[0] + 1 - 4)[0]
        if before <= skip < before + isize:
            holder = s
            break
        before += isize
    assert holder is not None and holder > 0   # (the header takes several blocks)
    for n in (2, 8, 64):
        out = (C.c_uint64 * (n + 1))()
        assert capi.lib().slimm_host_bgzf_ranges(p.encode(), skip, n, out) == capi.OK
        offs = list(out)
        assert offs[0] == 0 and offs[n] == len(blob) == os.path.getsize(p)
        assert all(a <= b for a, b in zip(offs, offs[1:]))
        assert all(o in set(starts) or o == len(blob) for o in offs[1:n])
        assert min(offs[1:]) >= holder
