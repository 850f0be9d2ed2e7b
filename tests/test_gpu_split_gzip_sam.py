"""One gzip-compressed SAM file split at block starts over the members of a group (include/slimm_hip.h, "gzip SAM by byte
range"), below the command: SlimmGroup.push_split(form="gzip_sam") plans the ranges in bits (slimm_host_gzip_ranges),
announces every member's flags and bits, runs the window pass, hands the windows on (slimm_group_gzip_windows), runs the text
pass and stitches the cuts.  Every integer and the profile must be the oracle's, the members' counters must sum to the census
of the pure-Python walker (tests/sam_deflate.py), and what is no cut must be refused with SLIMM_E_SPLIT -- no verdict on the
file.  The inputs are small (SLIMM_FORCE gzip_chunk=2048: a range of a few KB still has several chunks), and the file also
runs on the host emulator (SLIMM_EMU=1).  Only directed inputs go to a device: no random damage."""
import os
import tempfile
import zlib

import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import SlimmGroup
from slimm_amd.synth import CONFIGS, make_workload
from tests import sam_deflate as D
from tests.bam_io import write_sam
from tests.cases import holes_case, tiny_case
from tests.helpers import assert_matches_oracle, assert_profiles_match
from tests.sam_gz import header_len
from tests.test_gpu_bam_decode import _named
from tests.test_split_gzip_plan import file_blocks, stored_block

pytestmark = pytest.mark.gpu

UNSORTED = "@HD\tVN:1.6\tSO:unsorted"
CASES = {
    "tiny": lambda: _named(tiny_case()),
    "holes": lambda: _named(holes_case()),
    "config1": lambda: _named(make_workload(CONFIGS["config1"], seed=41, n_records=4000)),
    "config1_shuffled": lambda: _named(make_workload(CONFIGS["config1"], seed=43, n_records=4000, shuffled=True)),
}
_made = {}


def case(name, tail_newline=True):
    """(the workload, the oracle's result, its SAM text): made once, never changed"""
    key = (name, tail_newline)
    if key not in _made:
        w = CASES[name]()
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "x.sam")
            write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, **({"hd": UNSORTED} if "shuffled" in name else {}))
            text = open(p, "rb").read()
        _made[key] = (w, run_workload(w, use_qnames=True), text if tail_newline else text[:-1])
    return _made[key]


def forced(monkeypatch, *keys):
    monkeypatch.setenv("SLIMM_FORCE", ",".join(("gzip_chunk=2048",) + keys))


def census(blob):
    bl = file_blocks(blob)
    return {"members": sum(1 for b in bl if b[2]), "stored_blocks": sum(1 for b in bl if b[1] == 0), "fixed_blocks": sum(1 for b in bl if b[1] == 1),
            "dynamic_blocks": sum(1 for b in bl if b[1] == 2), "text_bytes": sum(b[3] for b in bl)}


def dynamic_starts(blob):
    return [b[0] for b in file_blocks(blob) if b[1] == 2 and not b[2]]


def split_and_check(w, o, blob, skip, members, grouped=True, window=0, offsets=None):
    g = SlimmGroup(w, [0] * members, grouped=grouped)
    offs, counts = g.push_split(blob, "gzip_sam", skip=skip, window=window, offsets=offsets)
    assert sum(g.member(i).records_held()[0] for i in range(members)) == len(w.records)
    stats = [g.member(i).gzip_stats() for i in range(members)]
    assert g.get_profiles()
    s = g.member(0)
    assert_matches_oracle(s, o, bins=False)
    assert_profiles_match(s.write_abundance(), o.profile_tsv)
    g.close()
    assert offs[0] == 0 and offs[-1] == 8 * len(blob) and all(a <= b for a, b in zip(offs, offs[1:]))
    if offsets is None:
        assert set(offs[1:-1]) <= set(dynamic_starts(blob)) | {8 * len(blob)}, offs
    # the members' counters are their own, and sum to the walker's census: every block and every member counted once
    for key, want in census(blob).items():
        assert sum(t[key] for t in stats) == want, (key, want, [t[key] for t in stats])
    return offs, counts, stats


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("kind", ["default", "mem1", "rle", "sync", "members"])
@pytest.mark.parametrize("name", ["tiny", "holes", "config1", "config1_shuffled"])
def test_profiles_of_a_split_gzip_file(monkeypatch, name, kind, members):
    """The planner's cuts; once at the usual round size and once with gzip_round=1 (the ranges pushed in windows of 3 000
    bytes and decoded as far as they go at every push: blocks, headers and trailers wait for their bytes)."""
    w, o, text = case(name)
    blob = D.copy_of(text, kind)
    skip = header_len(text)
    bl = file_blocks(blob)
    holder = next(i for i, b in enumerate(bl) if b[4] + b[3] >= skip)
    cuts = [b[0] for b in bl[holder + 1:] if b[1] == 2 and not b[2]]   # (where the planner may cut: said by the walker)
    # member 1's even share starts no later than this bit: a cut at or behind it leaves two ranges that are not empty
    floor = bl[holder + 1][0] if holder + 1 < len(bl) else 8 * len(blob)
    must_cut = any(c >= floor + (8 * len(blob) - floor) // members + 1 for c in cuts)
    for keys, window in (((), 0), (("gzip_round=1",), 3_000)):
        forced(monkeypatch, *keys)
        try:
            offs, counts, _ = split_and_check(w, o, blob, skip, members, grouped="shuffled" not in name, window=window)
        except capi.SlimmError as e:   # (a block or two: the plan leaves member 0 all of the file, and that is said before a push)
            assert e.code == capi.E_INVALID and "a gzip stream is not cut by byte range" in str(e) and not must_cut, str(e)
            continue
        assert set(offs[1:-1]) <= set(cuts) | {8 * len(blob)}
        if len(cuts) >= 4 * members and name.startswith("config1") and members <= 4:
            assert min(counts) > 0 and len(set(offs)) == members + 1


@pytest.mark.parametrize("members", [3, 4])
def test_one_gzip_member_over_all_the_ranges(monkeypatch, members):
    """memLevel 1: one gzip member of some sixty dynamic blocks.  Its CRC register and its length are folded over every cut, and
    the member that reads the trailer counts it."""
    w, o, text = case("config1")
    forced(monkeypatch)
    offs, counts, stats = split_and_check(w, o, D.member(text, memLevel=1), header_len(text), members)
    assert len(set(offs)) == members + 1 and min(counts) > 0
    assert [t["members"] for t in stats] == [0] * (members - 1) + [1]
    assert all(t["resolved_bytes"] > 0 for t in stats[1:])   # (copies from the bytes the left neighbour's window pass handed over)


# ---- crafted streams -----------------------------------------------------------------------------------------------------
def same_as_one_context(w, blob, text, offsets):
    """The crafted member's text through one context as text, and through a group of len(offsets) - 1 members cut at
    `offsets`: the same integers.  Returns the members' gzip stats."""
    from slimm_amd.profiler import Slimm
    from tests.test_gpu_compressed_sam import integers

    def results(s):   # (what tests/helpers.py: assert_matches_oracle holds of a group's member 0: every integer but the bins)
        full = integers(s)
        return (full[0]["hits_count"], {k: v for k, v in full[1].items() if k != "nz_uniq_cov2"}, full[3], full[4], full[5], s.taxon_counts(0),
                s.children_pairs(0))

    assert zlib.decompress(blob, 31) == text
    s = Slimm.for_workload(w, device=0, grouped=False)
    s.set_reference_names(w.ref_names)
    n = s.push_sam_bytes(text)
    s.get_profiles()
    want = results(s)
    s.close()
    members = len(offsets) - 1
    g = SlimmGroup(w, [0] * members, grouped=False)
    g.push_split(blob, "gzip_sam", skip=0, offsets=offsets)
    assert sum(g.member(i).records_held()[0] for i in range(members)) == n
    stats = [g.member(i).gzip_stats() for i in range(members)]
    assert g.get_profiles()
    assert results(g.member(0)) == want
    g.close()
    assert sum(t["text_bytes"] for t in stats) == len(text)
    return stats


def test_crafted_copies_across_a_cut(monkeypatch):
    """The cut exactly on the crafted chunk's first bit: a copy of 512 bytes at distance 32 768 -- the farthest byte the left
    member's window holds --, and a copy whose source starts 20 bytes in front of the cut and runs 40 bytes behind it."""
    w, o, text = case("config1_shuffled")
    body = text[header_len(text):]
    forced(monkeypatch)
    blob, crafted, before = D.far_copy_member(body, w.ref_names[0].encode())
    stats = same_as_one_context(w, blob, crafted, [0, 8 * (10 + before), 8 * len(blob)])
    assert stats[1]["resolved_bytes"] == 512 and stats[1]["fixed_blocks"] == 2 and stats[1]["members"] == 1, stats
    blob, crafted, before = D.straddling_copy_member(body)
    stats = same_as_one_context(w, blob, crafted, [0, 8 * (10 + before), 8 * len(blob)])
    assert stats[1]["resolved_bytes"] == 20 and stats[0]["members"] == 0, stats


def test_a_middle_range_of_nothing_but_copies(monkeypatch):
    """Three ranges written with the fixed codes.  The middle one is two copies of the 20 000 to 32 768 bytes in front of it and
    nothing else -- every symbol of its final window is a marker into the bytes in front of it --, and the third range's first
    copy reaches into that window: what member 2 is handed comes from member 0's text through member 1's markers."""
    w, o, text = case("config1_shuffled")
    body = text[header_len(text):]
    lines = D._lines(body)
    P = b"".join(lines[:260])
    assert len(P) > 36_000
    starts, p = [], 0
    for ln in lines[:260]:
        starts.append(p)
        p += len(ln)
    a = min(s for s in starts if len(P) - s <= 32_768)
    L = len(P) - a
    assert 20_000 <= L <= 32_768
    f = D.FixedBlocks().begin().literals(P).end().align()
    cut1 = 8 * (10 + len(f.out))
    f.begin()
    left = 2 * L
    while left:
        k = min(258, left) if left - min(258, left) != 1 and left - min(258, left) != 2 else min(258, left) - 3
        f.match(k, L)
        left -= k
    f.end().align()
    cut2 = 8 * (10 + len(f.out))
    first = lines[starts.index(a)]
    assert 3 <= len(first) <= 258
    rest = b"".join(lines[260:300])
    f.begin(True).match(len(first), L).literals(rest).end().finish()
    crafted = P + P[a:] * 2 + first + rest
    deflate = f.bytes()
    assert zlib.decompress(deflate, -15) == crafted and 2 * L >= 32_768
    blob = D.gzip_frame(deflate, crafted)
    forced(monkeypatch)
    stats = same_as_one_context(w, blob, crafted, [0, cut1, cut2, 8 * len(blob)])
    assert stats[1]["resolved_bytes"] == 2 * L and stats[2]["resolved_bytes"] == len(first), stats
    assert [t["members"] for t in stats] == [0, 0, 1]


# ---- where the cuts lie --------------------------------------------------------------------------------------------------
def test_cuts_around_member_headers_and_trailers(monkeypatch):
    """Members back to back (tests/sam_deflate.py: three_members -- four, an empty one among them).  A cut right behind the
    fourth member's header, on its first block; a range from the first member's blocks to the fourth's with a trailer, two
    whole members and a header inside it."""
    w, o, text = case("config1")
    blob = D.three_members(text)
    skip = header_len(text)
    bl = file_blocks(blob)
    finals = [i for i, b in enumerate(bl) if b[2]]
    assert len(finals) == 4
    m4 = bl[finals[2] + 1:]                      # (the fourth member's blocks: dynamic, with stored ones from the flushes)
    m1 = bl[:finals[0]]
    assert m4[0][1] == 2 and not m4[0][2] and len(m1) > 6 and len(m4) > 6
    forced(monkeypatch)
    offs, counts, stats = split_and_check(w, o, blob, skip, 2, offsets=[0, m4[0][0], 8 * len(blob)])
    assert [t["members"] for t in stats] == [3, 1] and min(counts) > 0
    inside1 = next(b[0] for b in m1[len(m1) // 2:] if b[1] == 2)
    inside4 = next(b[0] for b in m4[len(m4) // 2:] if b[1] == 2 and not b[2])
    offs, counts, stats = split_and_check(w, o, blob, skip, 3, offsets=[0, inside1, inside4, 8 * len(blob)])
    assert [t["members"] for t in stats] == [0, 3, 1] and min(counts) > 0


def test_eight_members_over_a_few_blocks(monkeypatch):
    """More members than dynamic blocks: the later cuts are the file's end, and those members are empty."""
    w, o, text = case("tiny")
    blob = D.member(text, memLevel=1)
    assert 2 <= len(dynamic_starts(blob)) <= 6
    forced(monkeypatch)
    offs, counts, _ = split_and_check(w, o, blob, header_len(text), 8)
    assert sum(1 for a, b in zip(offs, offs[1:]) if a == b) >= 2 and offs[-2] == offs[-1] and counts[-1] == 0


@pytest.mark.parametrize("name", ["config1", "config1_shuffled"])
def test_last_line_without_newline(monkeypatch, name):
    """Only the file's last member ends a last line that lacks its newline -- or the stitch, when that member's range is empty."""
    w, o, text = case(name, tail_newline=False)
    assert not text.endswith(b"\n")
    forced(monkeypatch)
    blob = D.member(text, memLevel=1)
    offs, counts, _ = split_and_check(w, o, blob, header_len(text), 4, grouped="shuffled" not in name)
    assert counts[-1] > 0
    offs, counts, _ = split_and_check(w, o, blob, header_len(text), 3, grouped="shuffled" not in name, offsets=[0, offs[2], 8 * len(blob), 8 * len(blob)])
    assert counts[-1] == 0


# ---- what is refused -----------------------------------------------------------------------------------------------------
def group_error(w, blob, skip, members, offsets=None):
    g = SlimmGroup(w, [0] * members, grouped=True)
    with pytest.raises(capi.SlimmError) as e:
        g.push_split(blob, "gzip_sam", skip=skip, offsets=offsets)
    g.close()
    return e.value


def test_a_wrong_trailer_of_a_member_over_a_cut(monkeypatch):
    """The stitch folds the register and the length over the cuts and holds them against the trailer: the single context's words."""
    w, o, text = case("config1")
    forced(monkeypatch)
    for kw, words in ((dict(crc=zlib.crc32(text) ^ 1), "corrupt gzip stream (incorrect data check)"),
                      (dict(isize=len(text) + 1), "corrupt gzip stream (incorrect length check)")):
        blob = D.member(text, memLevel=1, **kw)
        for members in (2, 4):
            got = group_error(w, blob, header_len(text), members)
            assert got.code == capi.E_INVALID and words in str(got) and f"byte {len(blob) - 8}" in str(got), str(got)


@pytest.mark.parametrize("members", [2, 4])
def test_a_wrong_cut_is_refused(monkeypatch, members):
    """SLIMM_FORCE gzip_split_wrong_cut: the planner's second cut (of two members: its only one) lands one bit late."""
    w, o, text = case("config1")
    forced(monkeypatch, "gzip_split_wrong_cut")
    got = group_error(w, D.member(text, memLevel=1), header_len(text), members)
    assert got.code == capi.E_SPLIT, str(got)


def test_valid_blocks_inside_a_stored_block_are_no_cut(monkeypatch):
    """A whole valid run of small dynamic blocks as a stored block's bytes: a planner could take its first bit for a cut, and a
    member that starts there decodes it happily.  The member on the left, whose chain takes the stored block in one step,
    steps over the cut -- or, as here, lacks the stored block's bytes behind its range's end: SLIMM_E_SPLIT."""
    w, o, text = case("config1")
    skip = header_len(text)
    body = text[skip:]
    inner = D.raw_deflate(body[:30_000], memLevel=1, final=False)
    assert len(inner) < 65_000 and sum(1 for b in D.blocks(inner + D.FixedBlocks().begin(True).end().finish().bytes())[0] if b[1] == 2) > 5
    head = D.raw_deflate(text[:skip + 2_000], memLevel=1, final=False)
    deflate = head + stored_block(inner) + D.raw_deflate(body[2_000:], memLevel=1)
    whole = text[:skip + 2_000] + inner + body[2_000:]
    blob = D.gzip_frame(deflate, whole)
    assert zlib.decompress(blob, 31) == whole
    forced(monkeypatch)
    got = group_error(w, blob, skip, 2, offsets=[0, 8 * (10 + len(head) + 5), 8 * len(blob)])
    assert got.code == capi.E_SPLIT and ("steps over the range's end" in str(got) or "has not reached the range's end" in str(got)), str(got)


def test_a_truncated_last_range_and_a_stored_only_file(monkeypatch):
    w, o, text = case("config1")
    forced(monkeypatch)
    blob = D.member(text, memLevel=1)
    g = SlimmGroup(w, [0] * 3, grouped=True)
    offs, _ = g.push_split(blob, "gzip_sam", skip=header_len(text))
    g.close()
    for short in (blob[:-3], blob[:(offs[2] // 8 + len(blob)) // 2]):   # (inside the trailer; inside the last range's blocks)
        got = group_error(w, short, header_len(text), 3, offsets=offs[:3] + [8 * len(short)])
        assert got.code == capi.E_INVALID and "truncated gzip stream" in str(got), str(got)
    got = group_error(w, D.member(text, level=0), header_len(text), 4)
    assert got.code == capi.E_INVALID and "not cut by byte range" in str(got), str(got)


def test_the_planners_knobs(monkeypatch):
    """SLIMM_FORCE gzip_cut_search=100: a cut is given up 100 bytes behind its target, where blocks are some 150 bytes long -- a
    cut that is not found is the next one found or the file's end, the range in between is empty, and the result is the same.
    gzip_cut_blocks=1: one boundary passed is enough; on a real file the cuts are the usual ones.  gzip_split_floor: the
    command's floor (tests/test_cli_split_input_gzip.py)."""
    w, o, text = case("config1")
    blob = D.member(text, memLevel=1)
    forced(monkeypatch)
    usual, _, _ = split_and_check(w, o, blob, header_len(text), 4)
    forced(monkeypatch, "gzip_cut_blocks=1")
    offs, _, _ = split_and_check(w, o, blob, header_len(text), 4)
    assert offs == usual
    forced(monkeypatch, "gzip_cut_search=100")
    try:
        offs, counts, _ = split_and_check(w, o, blob, header_len(text), 4)
        assert offs != usual or len(set(offs)) == 5
    except capi.SlimmError as e:
        assert e.code == capi.E_INVALID and "not cut by byte range" in str(e)
    assert capi.lib().slimm_gzip_split_floor() == 32 << 20
    forced(monkeypatch, "gzip_split_floor=0")
    assert capi.lib().slimm_gzip_split_floor() == 0
