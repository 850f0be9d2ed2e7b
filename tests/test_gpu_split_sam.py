"""One SAM file -- plain text, or BGZF blocks of it -- split by byte range over the members of a group (include/slimm_hip.h,
"ONE FILE SPLIT BY BYTE RANGE"), below the command: SlimmGroup.push_split plans the ranges, gives every member the reference
names and its mid-file flags, pushes the ranges and stitches the cuts.  The text is cut anywhere, so nearly every range
starts inside a line: its head -- the bytes through the first newline -- is decoded by the member on its left.  Every integer
and the profile must be the oracle's.  (The inputs are small: the file also runs on the host emulator, SLIMM_EMU=1.)"""
import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd import capi
from slimm_amd.profiler import SlimmGroup
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.workload import Records, Workload
from tests.bam_io import write_bam, write_sam
from tests.cases import holes_case, tiny_case
from tests.helpers import assert_matches_oracle, assert_profiles_match, force
from tests.sam_gz import bgzf, header_len
from tests.test_gpu_bam_decode import _named

pytestmark = pytest.mark.gpu

CASES = {"tiny": tiny_case, "holes": holes_case, "config1": lambda: make_workload(CONFIGS["config1"], seed=41, n_records=4000)}


def sam_text(tmp_path, w, tail_newline=True) -> bytes:
    p = str(tmp_path / "x.sam")
    write_sam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
    text = open(p, "rb").read()
    return text if tail_newline else text[:-1]


def file_of(text: bytes, form: str, seed: int = 2, eof: bool = True):
    """(the file's bytes, the header skip its pushes take)"""
    skip = header_len(text)
    if form == "sam":
        return text, skip
    return bgzf(text, seed=seed, lo=100, hi=400, eof=eof), skip   # (blocks of a few hundred bytes: every member gets some)


def split_and_check(w, data, form, skip, members, window=0):
    o = run_workload(w, use_qnames=True)
    g = SlimmGroup(w, [0] * members, grouped=True)
    offs, counts = g.push_split(data, form, skip=skip, window=window)
    assert g.get_profiles()
    s = g.member(0)
    assert_matches_oracle(s, o, bins=False)
    assert_profiles_match(s.write_abundance(), o.profile_tsv)
    g.close()
    return offs, counts


@pytest.mark.parametrize("members", [2, 4, 8])
@pytest.mark.parametrize("form", ["sam", "bgzf_sam"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_split_sam_has_the_oracles_integers_and_profile(tmp_path, case, form, members):
    w = _named(CASES[case]())
    data, skip = file_of(sam_text(tmp_path, w), form)
    offs, counts = split_and_check(w, data, form, skip, members)
    if case == "config1":
        assert all(b > a for a, b in zip(offs, offs[1:]))   # (every member has bytes of its own)
        assert min(counts) > 0


@pytest.mark.parametrize("form", ["sam", "bgzf_sam"])
def test_split_sam_in_small_windows(tmp_path, form):
    """Ranges pushed in several windows: lines straddle them, and only a range's first window looks for the first line."""
    w = _named(CASES["config1"]())
    data, skip = file_of(sam_text(tmp_path, w), form)
    split_and_check(w, data, form, skip, 4, window=20_000)


@pytest.mark.parametrize("eof", [True, False])
@pytest.mark.parametrize("form", ["sam", "bgzf_sam"])
def test_split_sam_last_line_without_newline(tmp_path, form, eof):
    """Only the file's last member ends a last line that lacks its newline; a range that ends inside the file ends inside
    a line, and the member on its right ends that one."""
    w = _named(CASES["config1"]())
    data, skip = file_of(sam_text(tmp_path, w, tail_newline=False), form, eof=eof)
    split_and_check(w, data, form, skip, 4)
    split_and_check(w, data, form, skip, 8, window=30_000)


@pytest.mark.parametrize("form", ["sam", "bgzf_sam"])
def test_split_sam_one_read_over_every_cut(tmp_path, form):
    """Every record of the middle half of the file belongs to one read: its run crosses cuts and whole members, and ends
    up with the member that holds its start."""
    w = CASES["config1"]()
    r = w.records
    n = len(r.read_key)
    key = np.array(r.read_key, copy=True)
    key[n // 4:3 * n // 4] = key[n // 4]
    w = _named(Workload(w.ref_names, w.ref_len, w.taxonomy, Records(key, r.flag, r.ref_id, r.begin_pos, None, r.file_flag),
                        w.avg_read_len, w.options, w.name))
    data, skip = file_of(sam_text(tmp_path, w), form)
    split_and_check(w, data, form, skip, 8)


@pytest.mark.parametrize("form", ["sam", "bgzf_sam"])
def test_split_sam_more_members_than_lines(tmp_path, form):
    """Sixteen members for the tiny case: ranges of a few lines, ranges inside one line (all head) and -- BGZF -- empty
    ranges."""
    w = _named(tiny_case())
    data, skip = file_of(sam_text(tmp_path, w), form, seed=5)
    split_and_check(w, data, form, skip, 16)


@pytest.mark.parametrize("eof", [True, False])
def test_split_bgzf_sam_last_range_without_text_and_no_last_newline(tmp_path, eof):
    """One block of alignment lines for four members, the last line without its newline: the file's last range holds the
    EOF block only (or nothing), so no member's own window ends that line -- the stitch does, in the member that holds it."""
    from tests.sam_gz import bgzf as blocks

    w = _named(tiny_case())
    text = sam_text(tmp_path, w, tail_newline=False)
    split_and_check(w, blocks(text, seed=1, lo=20_000, hi=60_000, eof=eof), "bgzf_sam", header_len(text), 4)


@pytest.mark.parametrize("form", ["sam", "bgzf_sam"])
def test_split_sam_head_off_by_one_is_refused(tmp_path, monkeypatch, form):
    """SLIMM_FORCE split_shift_guess: the head a member announces is one byte short, so the line across the cut does not
    end with it: SLIMM_E_SPLIT, not a wrong record."""
    w = _named(CASES["config1"]())
    data, skip = file_of(sam_text(tmp_path, w), form)
    g = SlimmGroup(w, [0, 0, 0], grouped=True)
    force(monkeypatch, split_shift_guess=1)
    with pytest.raises(capi.SlimmError) as e:
        g.push_split(data, form, skip=skip)
    assert e.value.code == capi.E_SPLIT
    g.close()


def test_split_bam_through_the_same_method(tmp_path):
    w = _named(CASES["config1"]())
    p = str(tmp_path / "x.bam")
    write_bam(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len, irregular_seed=5)
    from tests.test_split_ranges import header_bytes

    split_and_check(w, p, "bam", header_bytes(w), 4)
