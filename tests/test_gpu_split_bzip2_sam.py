"""One bzip2-compressed SAM file split by byte range over the members of a group (include/slimm_hip.h, "bzip2 SAM by byte
range"), below the command: SlimmGroup.push_split(form="bzip2_sam") plans the ranges at plain byte offsets, announces every
member's flags and file offsets, pushes its range plus the slack and stitches the cuts.  A block belongs to the member in whose
range the first bit of its magic lies; a member that starts inside the file finds its first block by itself, and the stitch
holds the members' chains of blocks against each other -- where they end and begin, the stream's level, the combined CRC --
before the text is joined as SAM text is.  Every integer and the profile must be the oracle's.  (The inputs are small: the file
also runs on the host emulator, SLIMM_EMU=1.)"""
import re

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import Slimm, SlimmGroup
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.workload import Records, Workload
from tests.bam_io import write_sam
from tests.cases import holes_case, tiny_case
from tests.helpers import assert_matches_oracle, assert_profiles_match, force
from tests.sam_bz2 import EOS_MAGIC, copies, flip_bit, header_len, magics, one_stream, streams
from tests.test_gpu_bam_decode import _named

pytestmark = pytest.mark.gpu

UNSORTED = "@HD\tVN:1.6\tSO:unsorted"
CASES = {
    "tiny": tiny_case,
    "holes": holes_case,
    "config1": lambda: make_workload(CONFIGS["config1"], seed=41, n_records=4000),
    "config1_shuffled": lambda: make_workload(CONFIGS["config1"], seed=43, n_records=4000, shuffled=True),
    "config1_long": lambda: make_workload(CONFIGS["config1"], seed=41, n_records=14000),
}
KINDS = ["level1", "level9", "streams", "header_blocks", "streams30k"]
_made = {}


def case(name, tail_newline=True):
    """(the named workload, the oracle's result, its SAM text): made once, never changed"""
    key = (name, tail_newline)
    if key not in _made:
        import os
        import tempfile

        w = _named(CASES[name]())
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "x.sam")
            write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, **({"hd": UNSORTED} if "shuffled" in name else {}))
            text = open(p, "rb").read()
        _made[key] = (w, run_workload(w, use_qnames=True), text if tail_newline else text[:-1])
    return _made[key]


def copy_of(text, kind):
    if kind == "streams30k":
        return streams(text, chunk=30000, levels=(1,), empty_at=2)
    return copies(text)[kind]


def starts_per_range(blob, offs):
    """block starts (the first bit of the magic) in every range"""
    bits = magics(blob)
    return [sum(1 for b in bits if a * 8 <= b < e * 8) for a, e in zip(offs, offs[1:])]


def split_and_check(w, o, blob, skip, members, grouped=True, window=0, offsets=None):
    g = SlimmGroup(w, [0] * members, grouped=grouped)
    offs, counts = g.push_split(blob, "bzip2_sam", skip=skip, window=window, offsets=offsets)
    assert sum(g.member(i).records_held()[0] for i in range(members)) == len(w.records)
    assert g.get_profiles()
    s = g.member(0)
    assert_matches_oracle(s, o, bins=False)
    assert_profiles_match(s.write_abundance(), o.profile_tsv)
    g.close()
    return offs, counts


@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["tiny", "holes", "config1"])
def test_split_bzip2_sam_has_the_oracles_integers_and_profile(name, kind, members):
    w, o, text = case(name)
    blob = copy_of(text, kind)
    offs, counts = split_and_check(w, o, blob, header_len(text), members)
    assert offs[0] == 0 and offs[-1] == len(blob)
    if name == "config1" and kind == "streams30k":   # (20 blocks and an empty stream: every range holds block starts)
        assert len(magics(blob)) == 20
        assert min(starts_per_range(blob, offs)) > 0
        assert min(counts) > 0
    if name == "config1" and kind == "level1" and members == 4:
        # three blocks of one stream: every cut lies inside a stream, and range 2 holds no block start -- an empty member
        assert magics(blob) == [32, 78946, 156101] and len(blob) == 21500
        # (the cuts divide the bytes behind the header's block: ranges 1 and 2 lie inside the second block)
        assert starts_per_range(blob, offs) == [2, 0, 0, 1]
        assert counts[1] == counts[2] == 0 and min(counts[0], counts[3]) > 0


def test_split_one_stream_at_the_quarters_of_the_file():
    """The same file cut at its quarters, [0, 5 375, 10 750, 16 125, 21 500] -- what the planner gives without a header to
    hold; with one, its cuts divide the bytes behind the header's block: [0, 12 776, 15 684, 18 592, 21 500].
    Range 2 = [10 750, 16 125) holds no block start and is an empty member; the first cut lies inside the block that
    holds the header, which is member 0's: the first bit of its magic is."""
    w, o, text = case("config1")
    blob = one_stream(text, 1)
    quarters = [len(blob) * i // 4 for i in range(5)]
    assert quarters[2:4] == [10750, 16125] and starts_per_range(blob, quarters) == [1, 1, 0, 1]
    offs, counts = split_and_check(w, o, blob, header_len(text), 4, offsets=quarters)
    assert offs == quarters and counts[2] == 0 and min(counts[0], counts[1], counts[3]) > 0


@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("kind", ["level1", "streams", "streams30k"])
@pytest.mark.parametrize("name", ["tiny", "holes", "config1_shuffled"])
def test_split_bzip2_sam_in_any_order(name, kind, members):
    """A group made for files in any order: the same cuts, then every member's records are dealt by key."""
    w, o, text = case(name)
    split_and_check(w, o, copy_of(text, kind), header_len(text), members, grouped=False)


@pytest.mark.parametrize("members", [3, 4])
def test_split_many_blocks_of_one_stream(members):
    """One stream of level 1 over every cut: no member but the first sees a stream header, none but the last a marker --
    the level and the combined CRC are the stitch's to check."""
    w, o, text = case("config1_long")
    blob = one_stream(text, 1)
    assert len(magics(blob)) >= 2 * members and len(magics(blob, EOS_MAGIC)) == 1
    offs, counts = split_and_check(w, o, blob, header_len(text), members)
    assert min(starts_per_range(blob, offs)) > 0 and min(counts) > 0


@pytest.mark.parametrize("round_bytes", [1, 3000])
@pytest.mark.parametrize("kind", ["level1", "streams30k"])
def test_split_bzip2_sam_in_small_windows(monkeypatch, kind, round_bytes):
    """SLIMM_FORCE bzip2_round: the range and its slack pushed in windows of 2 000 bytes and decoded as far as they go at
    every push (or every 3 000 bytes): a member's first block is found once its bytes are there, blocks wait for theirs."""
    w, o, text = case("config1")
    force(monkeypatch, bzip2_round=round_bytes)
    split_and_check(w, o, copy_of(text, kind), header_len(text), 4, window=2000)


@pytest.mark.parametrize("kind", ["level1", "streams30k"])
def test_false_magics_in_front_of_a_members_first_block_are_dropped(monkeypatch, kind):
    """SLIMM_FORCE bzip2_false_magics: candidates that are no blocks every 997 bits and inside every block -- those in front
    of a mid-file member's first block are decoded and dropped."""
    w, o, text = case("config1")
    force(monkeypatch, bzip2_false_magics=997)
    split_and_check(w, o, copy_of(text, kind), header_len(text), 4)
    split_and_check(w, o, copy_of(text, kind), header_len(text), 3, grouped=False, window=5000)


@pytest.mark.parametrize("kind", ["level1", "streams30k"])
def test_split_bzip2_sam_last_line_without_newline(kind):
    """Only the file's last member ends a last line that lacks its newline -- or the stitch, when that member is empty."""
    w, o, text = case("config1", tail_newline=False)
    blob = copy_of(text, kind)
    split_and_check(w, o, blob, header_len(text), 4)
    split_and_check(w, o, blob, header_len(text), 8, window=3000)
    # (the last range holds the end of the last block only: an empty member behind the text's end)
    wt, ot, tt = case("tiny", tail_newline=False)
    split_and_check(wt, ot, one_stream(tt, 9), header_len(tt), 3)


def test_split_bzip2_sam_one_read_over_every_cut(tmp_path):
    """Every record of the middle half of the file belongs to one read: its run crosses cuts and whole members."""
    w = CASES["config1"]()
    r = w.records
    n = len(r.read_key)
    key = np.array(r.read_key, copy=True)
    key[n // 4:3 * n // 4] = key[n // 4]
    w = _named(Workload(w.ref_names, w.ref_len, w.taxonomy, Records(key, r.flag, r.ref_id, r.begin_pos, None, r.file_flag),
                        w.avg_read_len, w.options, w.name))
    p = str(tmp_path / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(p, "rb").read()
    o = run_workload(w, use_qnames=True)
    split_and_check(w, o, streams(text, chunk=30000, levels=(1,), empty_at=2), header_len(text), 8)


@pytest.mark.parametrize("grouped", [True, False])
def test_split_bzip2_sam_more_members_than_blocks(grouped):
    """Sixteen members for the tiny case, one block: all ranges but one are empty members."""
    w, o, text = case("tiny")
    blob = one_stream(text, 9)
    assert len(magics(blob)) == 1
    offs, counts = split_and_check(w, o, blob, header_len(text), 16, grouped=grouped)
    assert sum(1 for c in counts if c) == 1 and starts_per_range(blob, offs)[0] == 1


# ---- what the stitch refuses -----------------------------------------------------------------------------------------------
MESSAGE = re.compile(r"bzip2-compressed input is not supported unless it decodes: .*")   # (behind "slimm_hip error N: ")


def one_context_error(w, blob, skip):
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(capi.SlimmError) as e:
        s.push_bzip2_sam_bytes(blob, skip=skip)
    s.close()
    return e.value


def group_error(w, blob, skip, members):
    g = SlimmGroup(w, [0] * members, grouped=True)
    with pytest.raises(capi.SlimmError) as e:
        g.push_split(blob, "bzip2_sam", skip=skip)
    g.close()
    return e.value


def test_combined_crc_of_a_stream_over_a_cut():
    """The stream spans the cut: the member on the right meets its marker with a partial value only, and the stitch puts the
    two together -- the same code and message as through one context."""
    w, o, text = case("config1")
    blob = one_stream(text, 1)
    eos = magics(blob, EOS_MAGIC)
    assert len(eos) == 1
    bad = flip_bit(blob, eos[0] + 48 + 1)
    one = one_context_error(w, bad, header_len(text))
    assert one.code == capi.E_INVALID and f"end-of-stream marker at byte {eos[0] // 8}: combined CRC mismatch" in str(one)
    for members in (2, 4):
        got = group_error(w, bad, header_len(text), members)
        assert got.code == one.code and MESSAGE.search(str(one)).group(0) in str(got), (members, str(got))


def test_block_crc_of_a_mid_file_members_first_block():
    """Nothing but its CRC says that a mid-file member's first block is one: the group reports SLIMM_E_SPLIT (the command then
    reads the file through member 0), one context reports the block."""
    w, o, text = case("config1")
    blob = one_stream(text, 1)
    third = magics(blob)[2]
    bad = flip_bit(blob, third + 48 + 9)
    one = one_context_error(w, bad, header_len(text))
    assert one.code == capi.E_INVALID and f"block at byte {third // 8}: block CRC mismatch" in str(one)
    got = group_error(w, bad, header_len(text), 2)   # (member 1's range holds the third block's start only)
    assert got.code == capi.E_SPLIT and f"at byte {third // 8}" in str(got), str(got)


@pytest.mark.parametrize("kind,members", [("level1", 2), ("streams30k", 4)])
def test_a_wrong_first_block_is_refused(monkeypatch, kind, members):
    """SLIMM_FORCE bzip2_split_wrong_first: a mid-file member passes over its first block or marker, so its chain starts
    behind the place where its left neighbour's ends: SLIMM_E_SPLIT, not wrong records."""
    w, o, text = case("config1")
    blob = copy_of(text, kind)
    force(monkeypatch, bzip2_split_wrong_first=1)
    got = group_error(w, blob, header_len(text), members)
    assert got.code == capi.E_SPLIT and "cut in front of member" in str(got), str(got)


def test_a_range_of_a_bzip2_file_needs_its_offsets():
    """slimm_set_input_mid_file alone does not do for bzip2: the cut is a matter of bits, told by slimm_set_input_range."""
    w, o, text = case("tiny")
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    s._check(s.L.slimm_set_input_mid_file(s.ctx, 1, 0))
    with pytest.raises(capi.SlimmError) as e:
        s.push_bzip2_sam_bytes(one_stream(text, 9))
    assert e.value.code == capi.E_INVALID and "slimm_set_input_range" in str(e.value)
    s.close()
