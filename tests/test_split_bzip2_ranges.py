"""slimm_host_bzip2_ranges (host only): the byte ranges of a bzip2-compressed SAM file that the members of a group read with
--split-input.  The cuts are plain byte offsets -- a block belongs to the range in which the first bit of its magic lies, and
the device finds the blocks --, the ranges cover the file once, and no cut lies in front of the end of the block that holds the
SAM header's last byte: member 0 holds the whole header."""
import bz2
import ctypes as C

import pytest

from slimm_amd import capi
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_sam
from tests.sam_bz2 import BLOCK_MAGIC, EOS_MAGIC, header_len, header_spanning, magics, one_stream, streams
from tests.test_gpu_bam_decode import _named


def ranges(path, n, skip=0):
    out = (C.c_uint64 * (n + 1))()
    assert capi.lib().slimm_host_bzip2_ranges(str(path).encode(), skip, n, out) == capi.OK
    return list(out)


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    w = _named(make_workload(CONFIGS["config1"], seed=41, n_records=4000))
    p = str(tmp_path_factory.mktemp("sam") / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    return open(p, "rb").read()


def header_block_end(blob, skip):
    """the first bit behind the block that holds decoded byte skip - 1, for a file whose header lies in streams of one block
    each: that block ends where its stream's end-of-stream marker begins"""
    pos, decoded = 0, 0
    while True:
        d = bz2.BZ2Decompressor()
        decoded += len(d.decompress(blob[pos:]))
        end = len(blob) - len(d.unused_data)
        if decoded >= skip:
            assert sum(1 for b in magics(blob, BLOCK_MAGIC) if pos * 8 <= b < end * 8) == 1
            return min(e for e in magics(blob, EOS_MAGIC) if e >= pos * 8)
        pos = end


@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 64])
@pytest.mark.parametrize("kind", ["level1", "streams", "header_blocks"])
def test_ranges_cover_the_file_and_never_decrease(tmp_path, text, kind, n):
    blob = {"level1": one_stream(text, 1), "streams": streams(text, chunk=30000, levels=(1,), empty_at=2),
            "header_blocks": header_spanning(text)}[kind]
    p = tmp_path / "x.sam.bz2"
    p.write_bytes(blob)
    for skip in (0, header_len(text)):
        offs = ranges(p, n, skip)
        assert offs[0] == 0 and offs[n] == len(blob)
        assert all(a <= b for a, b in zip(offs, offs[1:]))


def test_no_cut_in_front_of_the_end_of_the_headers_last_block(tmp_path, text):
    blob = header_spanning(text)
    skip = header_len(text)
    p = tmp_path / "x.sam.bz2"
    p.write_bytes(blob)
    # the header lies in several blocks (a stream each): the block that holds its last byte ends where the next element
    # -- its stream's end-of-stream marker -- begins
    end_bit = header_block_end(blob, skip)
    assert end_bit > magics(blob, BLOCK_MAGIC)[1]          # (really behind the first block)
    assert end_bit in magics(blob, EOS_MAGIC)
    for n in (2, 5, 64):
        offs = ranges(p, n, skip)
        assert min(offs[1:]) * 8 >= end_bit
        # ... and the bytes behind that block are divided evenly
        floor = (end_bit + 7) // 8
        assert offs[1:n] == [floor + (len(blob) - floor) * i // n for i in range(1, n)]
    # without a header to hold, the whole file is divided
    assert ranges(p, 4, 0) == [len(blob) * i // 4 for i in range(5)]


def test_more_ranges_than_bytes_gives_empty_ranges(tmp_path, text):
    blob = one_stream(text[:header_len(text) + 300], 1)
    p = tmp_path / "x.sam.bz2"
    p.write_bytes(blob)
    n = len(blob) + 50
    offs = ranges(p, n, header_len(text))
    assert offs[0] == 0 and offs[n] == len(blob)
    assert all(a <= b for a, b in zip(offs, offs[1:]))
    assert sum(1 for a, b in zip(offs, offs[1:]) if a == b) >= 50


def test_not_a_bzip2_file(tmp_path, text):
    out = (C.c_uint64 * 3)()
    L = capi.lib()
    assert L.slimm_host_bzip2_ranges(str(tmp_path / "missing.bz2").encode(), 0, 2, out) == capi.E_INVALID
    assert L.slimm_host_bzip2_ranges(str(tmp_path).encode(), 0, 2, out) == capi.E_INVALID   # (a directory)
    p = tmp_path / "x.sam"
    p.write_bytes(text)
    assert L.slimm_host_bzip2_ranges(str(p).encode(), 0, 2, out) == capi.E_INVALID            # (does not start "BZh")
    q = tmp_path / "short.bz2"
    q.write_bytes(one_stream(text, 1)[:2000])
    assert L.slimm_host_bzip2_ranges(str(q).encode(), header_len(text) + 200_000, 2, out) == capi.E_INVALID   # (ends inside the header's blocks)


def test_the_slack_is_what_the_formats_bounds_give():
    """A block of 900 000 bytes + end of block in symbols of at most 20 bits is 2 250 003 bytes; selectors, tables, the
    block's fixed fields and a marker with a stream header come on top; rounded up to 64 KiB."""
    slack = capi.lib().slimm_bzip2_split_slack()
    bits = (48 + 32 + 1 + 24 + 16 + 256 + 3 + 15) + 32767 * 6 + 6 * (5 + 258 * 39) + 900_001 * 20 + (48 + 32 + 7 + 32)
    assert slack % 65536 == 0 and 0 <= slack - (bits + 7) // 8 < 65536
