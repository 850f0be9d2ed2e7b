"""One xz-compressed SAM file split by byte range over the members of a group (include/slimm_hip.h, "xz SAM by byte range"),
below the command: SlimmGroup.push_split(form="xz_sam") plans the ranges from the file's indexes (slimm_host_xz_ranges), tells
every member its flags, its file offsets and the check kind of the stream its range starts in (slimm_host_xz_check_at ->
slimm_set_xz_range_check), pushes exactly its range and stitches the cuts.  A member starts at a stream header or at a block
and ends at a block's first byte or between streams -- anything else is SLIMM_E_SPLIT --, nothing in front of its range
exists for it, the blocks of a stream that lies over cuts are held against its index by the stitch, and the text is stitched
as SAM text is.  The records, counts and profile must be those of one context reading the same file.  The inputs: the
committed files of tests/golden/xz and containers written in Python (tests/sam_xz.py); they are small, and the file also runs
on the host emulator (SLIMM_EMU=1)."""
import struct
import zlib

import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import Slimm, SlimmGroup
from tests import sam_xz as X
from tests.helpers import assert_matches_oracle, assert_profiles_match
from tests.test_gpu_xz_sam import CENSUS

pytestmark = pytest.mark.gpu

WORDS = "xz-compressed input is not supported unless it decodes: "
_shared = {}


def case(tmp_path, grouped, n_records):
    """The workload, its text, the header's length, the oracle's run: made once per text, never changed."""
    key = (grouped, n_records)
    if key not in _shared:
        w = X.case_workload(grouped, n_records)
        text = X.case_text(tmp_path, grouped, n_records)
        _shared[key] = (w, text, X.header_len(text), run_workload(w, use_qnames=True))
    return _shared[key]


def one_context(w, grouped, blob, skip):
    """(records, xz_stats, profile) of one context reading the whole file: made once per file."""
    key = ("one", grouped, zlib.crc32(blob), len(blob))
    if key not in _shared:
        s = Slimm.for_workload(w, device=0, grouped=grouped)
        s.set_reference_names(w.ref_names)
        n = s.push_xz_sam_bytes(blob, skip=skip)
        st = s.xz_stats()
        assert s.get_profiles() is not None
        _shared[key] = (n, st, s.write_abundance())
        s.close()
    return _shared[key]


def blocks_at(blob):
    return [b["at"] for s in X.walk(blob) for b in s["blocks"]]


def legal_cuts(blob):
    out = []
    for s in X.walk(blob):
        out += [s["at"]] + [b["at"] for b in s["blocks"][1:]]
    return out + [len(blob)]


def split_and_check(c, grouped, blob, members, window=0, offsets=None):
    w, text, skip, o = c
    n_one, xz_one, profile_one = one_context(w, grouped, blob, skip)
    g = SlimmGroup(w, [0] * members, grouped=grouped)
    offs, counts = g.push_split(blob, "xz_sam", skip=skip, window=window, offsets=offsets)
    assert sum(g.member(i).records_held()[0] for i in range(members)) == len(w.records) == n_one
    stats = [g.member(i).xz_stats() for i in range(members)]
    assert g.get_profiles()
    s = g.member(0)
    assert_matches_oracle(s, o, bins=False)
    assert_profiles_match(s.write_abundance(), profile_one)
    assert_profiles_match(s.write_abundance(), o.profile_tsv)
    g.close()
    assert offs[0] == 0 and offs[-1] == len(blob) and all(a <= b for a, b in zip(offs, offs[1:]))
    if offsets is None:
        assert set(offs) <= set(legal_cuts(blob)) | {0}, offs
    # the members' counters are their own, and sum to the file's census -- which is one context's
    want = X.census(blob)
    for name, key in CENSUS.items():
        assert sum(t[name] for t in stats) == want[key] == xz_one[name], (name, [t[name] for t in stats], want[key])
    assert sum(t["match_bytes"] for t in stats) == xz_one["match_bytes"] and max(t["max_dist"] for t in stats) == xz_one["max_dist"]
    return offs, counts, stats


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 3, 4])
@pytest.mark.parametrize("kind", ["mt", "blocks"])
@pytest.mark.parametrize("grouped", [True, False])
def test_the_committed_files_of_fourteen_blocks(tmp_path, grouped, kind, members):
    """xz -T's blocks (sizes in their headers) and --block-size's (none), one stream: with three or four members a middle
    member sees neither the stream's header nor its index, and only the last one reads the index."""
    c = case(tmp_path, grouped, 3_000)
    blob = X.golden(X.GOLDEN_KINDS[kind][1].format("grouped" if grouped else "any"))
    offs, counts, stats = split_and_check(c, grouped, blob, members)
    assert len(set(offs)) == members + 1 and min(counts) > 0
    assert [t["streams"] for t in stats] == [1] + [0] * (members - 1)
    assert [t["index_records"] for t in stats] == [0] * (members - 1) + [len(blocks_at(blob))]
    assert all(t["blocks"] > 0 for t in stats)


@pytest.mark.parametrize("grouped", [True, False])
def test_three_blocks_for_four_members(tmp_path, grouped):
    """More members than cuts: the ranges behind the last cut are empty, and so are their members."""
    c = case(tmp_path, grouped, 1_000)
    blob = X.written_copies(c[1], "grouped" if grouped else "any")["reblocked"]
    offs, counts, stats = split_and_check(c, grouped, blob, 4)
    assert sum(1 for a, b in zip(offs, offs[1:]) if a == b) >= 1 and 0 in counts
    # ... and an empty range between two blocks of one stream: it hands the stream's blocks on
    at = blocks_at(blob)
    offs, counts, stats = split_and_check(c, grouped, blob, 4, offsets=[0, at[1], at[1], at[2], len(blob)])
    assert counts[1] == 0 and stats[1]["blocks"] == 0 and stats[3]["index_records"] == 3


@pytest.mark.parametrize("members", [2, 3, 4])
@pytest.mark.parametrize("grouped", [True, False])
def test_two_streams_with_padding(tmp_path, grouped, members):
    """The cut in front of stream 2 is its header: the padding in front of it is the left member's, and the right member reads
    the check kind itself."""
    c = case(tmp_path, grouped, 1_000)
    blob = X.written_copies(c[1], "grouped" if grouped else "any")["two_streams_padded"]
    one, two = X.walk(blob)
    split_and_check(c, grouped, blob, members)
    offs, counts, stats = split_and_check(c, grouped, blob, 3, offsets=[0, two["at"], two["blocks"][1]["at"], len(blob)])
    assert [t["streams"] for t in stats] == [1, 1, 0] and [t["index_records"] for t in stats] == [1, 0, 2]
    assert [t["check_crc64"] for t in stats] == [1, 0, 0] and [t["check_crc32"] for t in stats] == [0, 1, 1]


@pytest.mark.parametrize("members", [2, 3])
@pytest.mark.parametrize("check", [0, 1, 4, 10])
def test_the_told_check_sizes_the_field_behind_every_block(tmp_path, check, members):
    c = case(tmp_path, True, 1_000)
    blob = X.stream_of(X.part_blocks(c[1], "grouped"), check=check)
    at = blocks_at(blob)
    offs, counts, stats = split_and_check(c, True, blob, members, offsets=[0, at[1], len(blob)] if members == 2 else [0, at[1], at[2], len(blob)])
    name = {0: "check_none", 1: "check_crc32", 4: "check_crc64", 10: "sha256_unverified"}[check]
    assert [t[name] for t in stats] == [1] + ([2] if members == 2 else [1, 1])


@pytest.mark.parametrize("window", [0, 700])
@pytest.mark.parametrize("grouped", [True, False])
def test_a_header_over_two_blocks(tmp_path, monkeypatch, grouped, window):
    """Stored blocks of a few lines each, the header in the first two: member 0 holds both.  With windows of 700 bytes and
    SLIMM_FORCE xz_round=1 every push is walked as far as it goes, and a range's last push must leave nothing."""
    if window:
        monkeypatch.setenv("SLIMM_FORCE", "xz_round=1")
    c = case(tmp_path, grouped, 1_000)
    w, text, skip, o = c
    head = X.cut_lines(text[:2 * skip - 100], 2)
    parts = head + X.cut_lines(text[2 * skip - 100:], 9)
    assert len(head[0]) < skip < len(head[0]) + len(head[1])
    blob = X.stream_of([(X.block_header(), X.raw_chunks(p, 40_000), p) for p in parts], check=1)
    at = blocks_at(blob)
    for members in (2, 4):
        offs, counts, stats = split_and_check(c, grouped, blob, members, window=window)
        assert min(offs[1:]) >= at[2]


# ---- what is refused ---------------------------------------------------------------------------------------------------------
def group_error(c, blob, members, offsets=None, xz_checks=None, grouped=True):
    w, text, skip, o = c
    g = SlimmGroup(w, [0] * members, grouped=grouped)
    with pytest.raises(capi.SlimmError) as e:
        g.push_split(blob, "xz_sam", skip=skip, offsets=offsets, xz_checks=xz_checks)
        g.get_profiles()   # (never reached: no profile is delivered)
    g.close()
    return e.value


def test_a_range_of_an_xz_file_needs_its_offsets(tmp_path):
    """slimm_set_input_mid_file alone keeps today's refusal: an xz range is taken only where slimm_set_input_range says it lies."""
    w, text, skip, o = case(tmp_path, True, 1_000)
    blob = X.stored_chunks(text)
    for flags in ((1, 0), (0, 1)):
        s = Slimm.for_workload(w, device=0, grouped=True)
        s.set_reference_names(w.ref_names)
        s._check(s.L.slimm_set_input_mid_file(s.ctx, *flags))
        with pytest.raises(capi.SlimmError) as e:
            s.push_xz_sam_bytes(blob, skip=skip)
        assert e.value.code == capi.E_INVALID and "an xz stream is not cut by byte range" in str(e.value)
        assert "slimm_set_input_range" in str(e.value)
        s.close()


@pytest.mark.parametrize("where", ["start", "end"])
@pytest.mark.parametrize("shift", [4, -4])
@pytest.mark.parametrize("check", [0, 4])
def test_a_range_shifted_by_four_bytes_is_refused(tmp_path, check, shift, where):
    """The cut in front of member 1 (start) or behind it (end) four bytes off a block's first byte: the member that ends or
    starts there says so."""
    c = case(tmp_path, True, 1_000)
    blob = X.stream_of(X.part_blocks(c[1], "grouped"), check=check)
    at = blocks_at(blob)
    offs = [0, at[1] + shift, at[2], len(blob)] if where == "start" else [0, at[1], at[2] + shift, len(blob)]
    got = group_error(c, blob, 3, offsets=offs)
    assert got.code == capi.E_SPLIT, str(got)
    assert "does not end at a block boundary" in str(got) or "where no block starts" in str(got), str(got)
    # ... each side by itself: the range [at[1] + 4, at[2]) starts inside a block header, [at[1], at[2] + 4) ends inside one
    w, text, skip, o = c
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    lo, hi = (at[1] + 4, at[2]) if where == "start" else (at[1], at[2] + 4)
    s._check(s.L.slimm_set_input_mid_file(s.ctx, 1, 1))
    s._check(s.L.slimm_set_input_range(s.ctx, lo, hi))
    s._check(s.L.slimm_set_xz_range_check(s.ctx, check))
    with pytest.raises(capi.SlimmError) as e:
        s.push_xz_sam_bytes(blob[lo:hi])
    s.close()
    assert e.value.code == capi.E_SPLIT, str(e.value)
    assert ("where no block starts" if where == "start" else "does not end at a block boundary") in str(e.value), str(e.value)


@pytest.mark.parametrize("told,real", [(1, 4), (4, 1), (0, 4), (-1, 4), (4, 10)])
def test_a_wrong_told_check_delivers_no_profile(tmp_path, told, real):
    c = case(tmp_path, True, 1_000)
    blob = X.stream_of(X.part_blocks(c[1], "grouped"), check=real)
    at = blocks_at(blob)
    got = group_error(c, blob, 2, offsets=[0, at[1], len(blob)], xz_checks=[-1, told])
    assert got.code in (capi.E_SPLIT, capi.E_INVALID), str(got)
    # ... a kind told to a member that starts at a stream header: no stream lies over the cut in front of it
    blob = X.written_copies(c[1], "grouped")["two_streams_padded"]
    two = X.walk(blob)[1]
    got = group_error(c, blob, 2, offsets=[0, two["at"], len(blob)], xz_checks=[-1, 1])
    assert got.code in (capi.E_SPLIT, capi.E_INVALID), str(got)


def test_an_index_record_altered_for_the_left_members_block(tmp_path):
    """The index lies in member 1's range, block 0 in member 0's: member 1 checks its own two blocks' records and keeps the
    first, which the stitch holds against member 0's block."""
    c = case(tmp_path, True, 1_000)
    blob = X.stream_of(X.part_blocks(c[1], "grouped"), check=4)
    s = X.walk(blob)[0]
    records = list(s["records"])
    records[0] = (records[0][0], records[0][1] + 1)
    index = X.index_of(records)
    bad = blob[:s["index_at"]] + index + X.stream_footer(4, len(index))
    assert zlib.crc32(index[:-4]) == struct.unpack("<I", index[-4:])[0] and bad != blob
    at = blocks_at(blob)
    got = group_error(c, bad, 2, offsets=[0, at[1], len(blob)])
    assert got.code == capi.E_INVALID and f"index at byte {s['index_at']}: index does not match the blocks" in str(got), str(got)
    got = group_error(c, bad, 3, offsets=[0, at[1], at[2], len(blob)])   # (handed on through member 1, which has no index)
    assert got.code == capi.E_INVALID and "index does not match the blocks" in str(got), str(got)
    # ... one context says the same of the same file
    w, text, skip, o = c
    one = Slimm.for_workload(w, device=0, grouped=True)
    one.set_reference_names(w.ref_names)
    with pytest.raises(capi.SlimmError) as e:
        one.push_xz_sam_bytes(bad, skip=skip)
    one.close()
    assert f"index at byte {s['index_at']}: index does not match the blocks" in str(e.value)
    # a record fewer, or one more, than the blocks on the left
    for records in (s["records"][1:], [s["records"][0]] + s["records"]):
        index = X.index_of(records)
        bad = blob[:s["index_at"]] + index + X.stream_footer(4, len(index))
        got = group_error(c, bad, 2, offsets=[0, at[1], len(bad)], xz_checks=[-1, 4])   # (such an index plans nothing: the kinds are told)
        assert got.code == capi.E_INVALID and "index does not match the blocks" in str(got), str(got)


def test_a_check_byte_flipped_in_a_right_members_block_names_the_files_byte(tmp_path):
    c = case(tmp_path, True, 3_000)
    blob = X.golden(X.GOLDEN_KINDS["mt"][1].format("grouped"))
    g = SlimmGroup(c[0], [0] * 3, grouped=True)
    offs, _ = g.push_split(blob, "xz_sam", skip=c[2])
    g.close()
    b = [b for b in X.walk(blob)[0]["blocks"] if b["at"] > offs[2]][1]
    bad = bytearray(blob)
    bad[b["check_at"] + 2] ^= 0x20
    got = group_error(c, bytes(bad), 3)
    assert got.code == capi.E_INVALID and WORDS + f"block at byte {b['at']}: check mismatch" in str(got), str(got)
