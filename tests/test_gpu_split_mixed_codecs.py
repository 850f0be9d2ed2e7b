"""A group whose members hold ranges of DIFFERENT codecs (include/slimm_hip.h, "ONE FILE SPLIT BY BYTE RANGE"): member 0's
codec picks the check that slimm_group_stitch_ranges runs over every member (windows.h: StreamCodec::stitch), so a zstd range
beside a bzip2 range is refused by the check of whichever came first.  Two members on one device, the `tiny` case, every range
announced as its own codec requires; nothing is stitched, and nothing is decoded that a good file would not decode.  (Small:
the file also runs on the host emulator, SLIMM_EMU=1.)"""
import pytest

from slimm_amd import capi
from slimm_amd.profiler import SlimmGroup
from tests import sam_zst as Z
from tests.sam_bz2 import one_stream
from tests.sam_gz import header_len
from tests.test_gpu_split_zstd_sam import case

pytestmark = pytest.mark.gpu


def push_range(g, i, form, blob, begin, end, skip):
    """Member i of two: the range [begin, end) of `blob`, announced and pushed as SlimmGroup.push_split does for `form`."""
    m = g.member(i)
    m.set_reference_names(g.w.ref_names)
    m._check(g.L.slimm_set_input_mid_file(m.ctx, 1 if i > 0 else 0, 1 if i + 1 < 2 else 0))
    m._check(g.L.slimm_set_input_size_hint(m.ctx, end - begin))
    m._check(g.L.slimm_set_input_range(m.ctx, begin, end))
    if form == "bzip2_sam":
        return m.push_bzip2_sam_bytes(blob[begin:end + g.L.slimm_bzip2_split_slack()], skip=skip if i == 0 else 0)
    return m.push_zstd_sam_bytes(blob[begin:end], skip=skip if i == 0 else 0)


def stitch_error(first):
    w, _, text = case("tiny")
    lines = Z.cut_lines(text, 2)
    zst = Z.raw_frame(lines[0]) + Z.raw_frame(lines[1])
    bz2 = one_stream(text, 1)
    cut = {"zstd_sam": len(Z.raw_frame(lines[0])), "bzip2_sam": len(bz2) // 2}   # (a frame start; any byte inside the one block)
    blob = {"zstd_sam": zst, "bzip2_sam": bz2}
    second = "bzip2_sam" if first == "zstd_sam" else "zstd_sam"
    g = SlimmGroup(w, [0, 0], grouped=True)
    push_range(g, 0, first, blob[first], 0, cut[first], header_len(text))
    push_range(g, 1, second, blob[second], cut[second], len(blob[second]), 0)
    with pytest.raises(capi.SlimmError) as e:
        g._check(g.L.slimm_group_stitch_ranges(g.g))
    g.close()
    return e.value


def test_zstd_first_refuses_the_bzip2_member():
    got = stitch_error("zstd_sam")
    assert got.code == capi.E_INVALID, str(got)
    assert "member 1 (device 0): the frames of a range: a range of a zstd file: slimm_set_input_range tells where it lies" in str(got), str(got)


def test_bzip2_first_finds_no_block_behind_member_0():
    got = stitch_error("bzip2_sam")
    assert got.code == capi.E_SPLIT, str(got)
    assert "cut in front of member 0: bzip2: the chain of member 0 ends at bit " in str(got), str(got)
    assert str(got).endswith(", and no range behind it holds a block"), str(got)
