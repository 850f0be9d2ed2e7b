"""One zstd-compressed SAM file split by byte range over the members of a group (include/slimm_hip.h, "zstd SAM by byte
range"), below the command: SlimmGroup.push_split(form="zstd_sam") plans the ranges at frame starts (slimm_host_zstd_ranges),
announces every member's flags and file offsets, pushes exactly its range and stitches the cuts.  A member starts at a frame
and ends between frames -- anything else is SLIMM_E_SPLIT --, nothing in front of its range exists for it, and the text it
decodes is stitched as SAM text is.  Every integer and the profile must be the oracle's.  The inputs: the committed
multi-frame files of tests/golden/zstd_frames and frames written in Python (tests/sam_zst.py); they are small, and the file
also runs on the host emulator (SLIMM_EMU=1)."""
import os
import re
import tempfile

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import Slimm, SlimmGroup
from slimm_amd.synth import CONFIGS, make_workload
from tests import sam_zst as Z
from tests.bam_io import write_sam
from tests.cases import holes_case, q18_apart_case, tiny_case
from tests.helpers import assert_matches_oracle, assert_profiles_match, force
from tests.sam_gz import header_len
from tests.test_cli_split_input import one_run
from tests.test_gpu_bam_decode import _named

pytestmark = pytest.mark.gpu

FRAMES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_frames")
UNSORTED = "@HD\tVN:1.6\tSO:unsorted"
CASES = {
    "tiny": lambda: _named(tiny_case()),
    "holes": lambda: _named(holes_case()),
    "config1": lambda: _named(make_workload(CONFIGS["config1"], seed=41, n_records=4000)),
    "config1_shuffled": lambda: _named(make_workload(CONFIGS["config1"], seed=43, n_records=4000, shuffled=True)),
    "golden_grouped": lambda: Z.case_workload(True, 3_000),     # (the text of the committed files)
    "golden_any": lambda: Z.case_workload(False, 3_000),
    "q18_apart": q18_apart_case,
    # a name run of 2 000 records over the middle of the file: it crosses cuts and whole members
    "long_run": lambda: one_run(make_workload(CONFIGS["config1"], seed=41, n_records=4000), 1000, 3000),
}
_made = {}


def case(name, tail_newline=True):
    """(the workload, the oracle's result, its SAM text): made once, never changed"""
    key = (name, tail_newline)
    if key not in _made:
        w = CASES[name]()
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "x.sam")
            if name.startswith("golden"):
                text = Z.case_text(d, name == "golden_grouped", 3_000)
            else:
                write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, **({"hd": UNSORTED} if "shuffled" in name else {}))
                text = open(p, "rb").read()
        _made[key] = (w, run_workload(w, use_qnames=True), text if tail_newline else text[:-1])
    return _made[key]


def frames_of(text, step, extras=True):
    """Frames of `step` bytes of text each in raw blocks, every one with its checksum; behind the second an empty frame, behind
    the first and third a skippable one."""
    out = []
    for k, i in enumerate(range(0, len(text), step)):
        out.append(Z.raw_frame(text[i:i + step], step=min(step, 50_000)))
        if extras and k == 1:
            out.append(Z.raw_frame(b""))
        if extras and k in (0, 2):
            out.append(Z.skippable())
    return b"".join(out)


def three_frames(text):
    a, b, c = Z.cut_lines(text, 3)
    return Z.raw_frame(a) + Z.raw_frame(b, rle=True) + Z.raw_frame(c, content_size=False)


def golden(tag, level):
    return open(os.path.join(FRAMES, f"config1_{tag}_frames_l{level}.sam.zst"), "rb").read()


def starts(blob):
    return [f["at"] for f in Z.walk(blob)] + [len(blob)]


def split_and_check(w, o, blob, skip, members, grouped=True, window=0, offsets=None):
    g = SlimmGroup(w, [0] * members, grouped=grouped)
    offs, counts = g.push_split(blob, "zstd_sam", skip=skip, window=window, offsets=offsets)
    assert sum(g.member(i).records_held()[0] for i in range(members)) == len(w.records)
    stats = [g.member(i).zstd_stats() for i in range(members)]
    assert g.get_profiles()
    s = g.member(0)
    assert_matches_oracle(s, o, bins=False)
    assert_profiles_match(s.write_abundance(), o.profile_tsv)
    g.close()
    assert offs[0] == 0 and offs[-1] == len(blob) and all(a <= b for a, b in zip(offs, offs[1:]))
    if offsets is None:
        assert set(offs) <= set(starts(blob)), offs
    # the members' counters are their own, and sum to the file's census
    c = Z.census(blob)
    assert sum(t["frames"] for t in stats) == c["frames"] and sum(t["skippable"] for t in stats) == c["skippable"]
    assert sum(t["raw_blocks"] + t["rle_blocks"] + t["compressed_blocks"] for t in stats) == c["raw"] + c["rle"] + c["compressed"]
    assert sum(t["compressed_bytes"] for t in stats) == len(blob)
    return offs, counts


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("level", [3, 19])
@pytest.mark.parametrize("tag", ["grouped", "any"])
def test_the_committed_multi_frame_files(tag, level, members):
    """Seven frames of libzstd's, cut inside lines, a skippable frame in front of each."""
    w, o, text = case("golden_" + tag)
    blob = golden(tag, level)
    offs, counts = split_and_check(w, o, blob, header_len(text), members, grouped=tag == "grouped")
    assert set(offs) <= set(starts(blob))   # (in front of a skippable frame, or of the frame behind it)
    if members <= 4:
        assert min(counts) > 0 and len(set(offs)) == members + 1


@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("name", ["tiny", "holes", "config1", "config1_shuffled"])
def test_raw_frames_of_30000_bytes(name, members):
    w, o, text = case(name)
    blob = frames_of(text, 30_000)
    offs, counts = split_and_check(w, o, blob, header_len(text), members, grouped="shuffled" not in name)
    if name.startswith("config1") and members <= 4:
        assert min(counts) > 0


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("members", [2, 4, 8])
def test_frames_of_40_bytes_hold_no_newline(members, grouped):
    """Frames shorter than a line: a range may be all head, and so may its neighbour -- their bytes are handed on to the left."""
    w, o, text = case("tiny")
    blob = frames_of(text, 40, extras=False)
    bare = [b"\n" not in text[i:i + 40] for i in range(0, len(text), 40)]   # (frame k holds text[40 k, 40 k + 40))
    assert sum(bare) > len(bare) // 2                                        # (lines are longer than that)
    split_and_check(w, o, blob, header_len(text), members, grouped=grouped)
    # ... and ranges of ONE frame each around a cut: members 1 and 2 are both all head
    at = starts(blob)
    k = next(k for k in range(len(bare) // 2, len(bare) - 2) if bare[k] and bare[k + 1])
    split_and_check(w, o, blob, header_len(text), 4, grouped=grouped, offsets=[0, at[k], at[k + 1], at[k + 2], len(blob)])


@pytest.mark.parametrize("name", ["tiny", "config1", "config1_shuffled"])
def test_three_frames_for_eight_members(name):
    """More members than frames: the planner's later cuts are the file's size, and those members are empty."""
    w, o, text = case(name)
    blob = three_frames(text)
    offs, counts = split_and_check(w, o, blob, header_len(text), 8, grouped="shuffled" not in name)
    assert sum(1 for a, b in zip(offs, offs[1:]) if a == b) >= 5 and sum(1 for c in counts if c) <= 3


# ---- where the cuts lie ------------------------------------------------------------------------------------------------------
def test_a_cut_on_a_line_start_and_a_range_of_no_text():
    """offsets=: member 1's range holds a skippable and an empty frame only -- no text: an empty member --, and member 2
    starts exactly on a line start: its head is that whole line."""
    w, o, text = case("config1")
    lines = text.split(b"\n")
    a = b"\n".join(lines[:1500]) + b"\n"
    b = b"\n".join(lines[1500:3000]) + b"\n"
    c = text[len(a) + len(b):]
    fa, gap, fb, fc = Z.raw_frame(a), Z.skippable() + Z.raw_frame(b""), Z.raw_frame(b), Z.raw_frame(c)
    blob = fa + gap + fb + fc
    cuts = [0, len(fa), len(fa) + len(gap), len(fa) + len(gap) + len(fb), len(blob)]
    offs, counts = split_and_check(w, o, blob, header_len(text), 4, offsets=cuts)
    assert counts[1] == 0 and min(counts[0], counts[2], counts[3]) > 0
    split_and_check(w, o, blob, header_len(text), 4)   # (and where the planner cuts it)


@pytest.mark.parametrize("grouped", [True, False])
def test_last_line_without_newline(grouped):
    """Only the file's last member ends a last line that lacks its newline -- or the stitch, when that member holds no text."""
    w, o, text = case("config1" if grouped else "config1_shuffled", tail_newline=False)
    assert not text.endswith(b"\n")
    blob = frames_of(text, 30_000)
    offs, counts = split_and_check(w, o, blob, header_len(text), 4, grouped=grouped)
    assert counts[-1] > 0
    # the last member's range: a skippable frame only (no text), or nothing at all
    tail = blob + Z.skippable(b"the end")
    at = starts(blob)
    split_and_check(w, o, tail, header_len(text), 3, grouped=grouped, offsets=[0, at[len(at) // 2], len(blob), len(tail)])
    offs, counts = split_and_check(w, o, three_frames(text), header_len(text), 8, grouped=grouped)
    assert offs[-2] == offs[-1] and counts[-1] == 0


@pytest.mark.parametrize("kind", ["raw30k", "golden_l3"])
def test_small_rounds(monkeypatch, kind):
    """SLIMM_FORCE zstd_round=1: the ranges pushed in windows of 2 000 bytes and decoded as far as they go at every push --
    frame headers, block headers, blocks and checksums wait for their bytes; a range's last push must leave nothing."""
    force(monkeypatch, zstd_round=1)
    if kind == "raw30k":
        w, o, text = case("config1")
        blob = frames_of(text, 30_000)
    else:
        w, o, text = case("golden_grouped")
        blob = golden("grouped", 3)
    split_and_check(w, o, blob, header_len(text), 4, window=2000)


def test_a_bounded_search_leaves_empty_members(monkeypatch):
    """SLIMM_FORCE zstd_cut_search=1000 over frames of 30 000 bytes: cuts that are not found become the next one found or the
    file's size, the ranges in between are empty, and the result is the same."""
    w, o, text = case("config1")
    blob = frames_of(text, 30_000)
    force(monkeypatch, zstd_cut_search=1000)
    offs, counts = split_and_check(w, o, blob, header_len(text), 4)
    assert len(set(offs)) < 5 and 0 in counts
    assert capi.lib().slimm_zstd_split_floor() == 32 << 20      # (the command's floor: tests/test_cli_split_input_zstd.py)
    force(monkeypatch, zstd_split_floor=0)
    assert capi.lib().slimm_zstd_split_floor() == 0


# ---- Q18 and long runs -------------------------------------------------------------------------------------------------------
def test_q18_runs_apart_ask_for_the_any_order_path():
    """The members' Q18 counts are summed by the stitch: SLIMM_E_REGROUP as for one context; in any order the oracle's."""
    w, o, text = case("q18_apart")
    blob = frames_of(text, 300, extras=False)
    g = SlimmGroup(w, [0] * 4, grouped=True)
    with pytest.raises(capi.SlimmError) as e:
        g.push_split(blob, "zstd_sam", skip=header_len(text))
    g.close()
    assert e.value.code == capi.E_REGROUP
    split_and_check(w, o, blob, header_len(text), 4, grouped=False)


@pytest.mark.parametrize("members", [4, 8])
def test_a_name_run_over_cuts_and_whole_members(members):
    w, o, text = case("long_run")
    split_and_check(w, o, frames_of(text, 30_000), header_len(text), members)


# ---- what is refused ---------------------------------------------------------------------------------------------------------
MESSAGE = re.compile(r"zstd-compressed input is not supported unless it decodes: .*")   # (behind "slimm_hip error N: ")


def group_error(w, blob, skip, members, offsets=None):
    g = SlimmGroup(w, [0] * members, grouped=True)
    with pytest.raises(capi.SlimmError) as e:
        g.push_split(blob, "zstd_sam", skip=skip, offsets=offsets)
    g.close()
    return e.value


def test_a_wrong_checksum_in_member_2_names_the_files_byte():
    """The member that owns the frame checks its content checksum, and names the frame's byte in the FILE, in the words one
    context has for that file."""
    w, o, text = case("config1")
    blob = frames_of(text, 30_000)
    g = SlimmGroup(w, [0] * 4, grouped=True)
    offs, _ = g.push_split(blob, "zstd_sam", skip=header_len(text))
    g.close()
    f = [f for f in Z.walk(blob) if not f["skippable"] and f["checksum_at"] and offs[2] <= f["at"] < offs[3] and f["content_size"]][0]
    bad = bytearray(blob)
    bad[f["checksum_at"] + 1] ^= 0x10
    bad = bytes(bad)
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(capi.SlimmError) as e:
        s.push_zstd_sam_bytes(bad, skip=header_len(text))
    s.close()
    one = e.value
    assert one.code == capi.E_INVALID and f"frame at byte {f['at']}: content checksum mismatch" in str(one)
    got = group_error(w, bad, header_len(text), 4)
    assert got.code == capi.E_INVALID and MESSAGE.search(str(one)).group(0) in str(got), str(got)


@pytest.mark.parametrize("members", [2, 4])
def test_a_wrong_cut_is_refused(monkeypatch, members):
    """SLIMM_FORCE zstd_split_wrong_cut: the planner's second cut (of two members: its only one) lands one byte late."""
    w, o, text = case("config1")
    blob = frames_of(text, 30_000)
    force(monkeypatch, zstd_split_wrong_cut=1)
    got = group_error(w, blob, header_len(text), members)
    assert got.code == capi.E_SPLIT, str(got)
    assert "no frame starts" in str(got) or "does not end at a frame boundary" in str(got), str(got)


def test_a_cut_inside_a_frame_is_refused():
    w, o, text = case("config1")
    blob = frames_of(text, 30_000)
    at = starts(blob)
    inside = at[5] + 1000
    assert inside not in at
    got = group_error(w, blob, header_len(text), 2, offsets=[0, inside, len(blob)])
    assert got.code == capi.E_SPLIT and "does not end at a frame boundary" in str(got), str(got)
    # ... from the right member's start when the left one is fine: the cut one byte behind a frame start
    got = group_error(w, blob, header_len(text), 3, offsets=[0, at[3], at[5] + 1, len(blob)])
    assert got.code == capi.E_SPLIT, str(got)


def test_a_range_of_a_zstd_file_needs_its_offsets():
    """slimm_set_input_mid_file alone keeps today's refusal: a zstd range is taken only where slimm_set_input_range says it lies."""
    w, o, text = case("tiny")
    for flags in ((1, 0), (0, 1)):
        s = Slimm.for_workload(w, device=0, grouped=True)
        s.set_reference_names(w.ref_names)
        s._check(s.L.slimm_set_input_mid_file(s.ctx, *flags))
        with pytest.raises(capi.SlimmError) as e:
            s.push_zstd_sam_bytes(Z.raw_frame(text))
        assert e.value.code == capi.E_INVALID and "a zstd stream is not cut by byte range" in str(e.value)
        assert "slimm_set_input_range" in str(e.value)
        s.close()
