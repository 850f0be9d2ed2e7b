"""The directed bzip2 and deflate inputs (tests/bzip2_directed.py, tests/deflate_directed.py: one path family of the block
decoders each, shown to reach it by tests/test_codec_paths_bzip2_deflate.py) on a real MI355X.  Each bzip2 input goes through
slimm_push_bzip2_sam_bytes whole, and cut at random offsets with a round per push; each gzip input through
slimm_push_gzip_sam_bytes under its force key -- the crafted block at a chunk start -- and once more cut at random offsets
with a round per push; each deflate stream once more as a BGZF block through slimm_push_bgzf_sam_blocks and through both
paths of slimm_bgzf_inflate_with.  The partials must equal those of slimm_push_sam_bytes on the plain text, the profile the
oracle's, and what the decoders report of the input -- streams, blocks and false magics of bzip2; blocks by type, chunks and
the bytes resolved from in front of their chunk of gzip -- the census of tests/bzip2_paths.py and tests/deflate_paths.py.
Every input carries a check the decoder verifies (block CRC; CRC32 and ISIZE), which is what turns one wrong byte of the text
into a failure.  Every invalid variant is refused in its words.  The inputs are small (50 records): the file also runs on the
host emulator (SLIMM_EMU=1)."""
import re
import tempfile

import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from tests import bzip2_directed, bzip2_paths, deflate_directed, deflate_paths, sam_bz2, sam_xz as X
from tests.helpers import assert_matches_oracle
from tests.test_gpu_bgzf_inflate import _inflate_with
from tests.test_gpu_compressed_sam import profile_of
from tests.test_gpu_xz_sam import forced, random_cuts

pytestmark = pytest.mark.gpu

RECORDS = 50
_shared = {}


def case():
    """The workload, the plain text's profile, the oracle's run and the directed inputs of both codecs: made once."""
    if not _shared:
        w = X.case_workload(True, RECORDS)
        with tempfile.TemporaryDirectory() as d:
            text = X.case_text(d, True, RECORDS)
        skip = X.header_len(text)
        s, want = profile_of(w, True, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        gz = deflate_directed.INPUTS(text[:skip], text[skip:])
        _shared.update(w=w, want=want, oracle=run_workload(w, use_qnames=True), bzip2=bzip2_directed.INPUTS(text[:skip], text[skip:]), gzip=gz,
                       bgzf=deflate_directed.as_bgzf(gz), bad_bzip2=bzip2_directed.INVALID(text[:skip], text[skip:]),
                       bad_gzip=deflate_directed.INVALID(text[:skip], text[skip:]), census={})
    return _shared


def census_of(codec, name, chunk_bytes=None):
    c = case()
    key = (codec, name, chunk_bytes)
    if key not in c["census"]:
        blob = c[codec][name][0]
        if codec == "bzip2":
            c["census"][key] = bzip2_paths.decode(blob)[1]
        else:
            c["census"][key] = deflate_paths.decode(blob, deflate_paths.chunk_starts(blob, chunk_bytes) if chunk_bytes else ())[1]
    return c["census"][key]


def cuts_of(blob, cut):
    return random_cuts(len(blob), 7, 1, max(2_000, len(blob) // 20)) if cut == "random" else []


def trace_counts(err: str):
    m = re.findall(r"\[push bzip2\] (\d+) streams, (\d+) blocks in \d+ batches, (\d+) false magics", err)
    assert m, err[-500:]
    return tuple(int(v) for v in m[-1])


@pytest.mark.parametrize("cut,force", [("one", ""), ("random", bzip2_directed.FORCE)])
@pytest.mark.parametrize("name", bzip2_directed.NAMES)
def test_directed_bzip2_inputs_give_the_partials_of_the_text(monkeypatch, capfd, name, cut, force):
    c = case()
    blob, text, skip, _, round_per_push = c["bzip2"][name]
    assert round_per_push == bzip2_directed.FORCE
    forced(monkeypatch, force)
    monkeypatch.setenv("SLIMM_TRACE", "push")
    capfd.readouterr()
    s, got = profile_of(c["w"], True, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    assert got == c["want"]
    assert_matches_oracle(s, c["oracle"])
    s.close()
    census = census_of("bzip2", name)
    blocks = census["count:blocks"]
    assert trace_counts(capfd.readouterr().err) == (census["count:streams"], blocks, len(sam_bz2.magics(blob)) - blocks)


@pytest.mark.parametrize("cut", ["one", "random"])
@pytest.mark.parametrize("name", deflate_directed.NAMES)
def test_directed_gzip_inputs_give_the_partials_of_the_text(monkeypatch, name, cut):
    c = case()
    blob, text, skip, _, force = c["gzip"][name]
    forced(monkeypatch, ",".join(f for f in (force, "gzip_round=1" if cut == "random" else None) if f))
    s, got = profile_of(c["w"], True, lambda s: s.push_gzip_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    st = s.gzip_stats()
    assert got == c["want"]
    assert_matches_oracle(s, c["oracle"])
    s.close()
    chunk = int(force.split("=")[1]) if force else None
    census = census_of("gzip", name, chunk)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob) and st["members"] == 1, st
    assert (st["stored_blocks"], st["fixed_blocks"], st["dynamic_blocks"]) == (census["count:stored"], census["count:fixed"], census["count:dynamic"]), st
    assert st["dropped"] == 0, st
    if force:
        assert st["chunks"] >= 2, st
    if cut == "one":   # (one round: the chunk starts are the member's first block and the candidates the force key picks)
        assert st["chunks"] == census["count:chunks"], (st, census["count:chunks"])
        assert st["resolved_bytes"] == census["bytes:from_in_front_of_chunk"], (st, census["bytes:from_in_front_of_chunk"])
    else:
        assert st["rounds"] > 1, st


@pytest.mark.parametrize("name", [n for n in deflate_directed.NAMES if n not in deflate_directed.NOT_IN_BGZF])
def test_directed_deflate_streams_in_bgzf_blocks_give_the_text_and_its_partials(monkeypatch, name):
    c = case()
    blocks, text, skip = c["bgzf"][name]
    forced(monkeypatch, None)
    s, got = profile_of(c["w"], True, lambda s: s.push_bgzf_sam_blocks(blocks, skip=skip))
    assert got == c["want"]
    assert_matches_oracle(s, c["oracle"])
    s.close()
    # both inflate paths give the text; the two-phase kernels hand over only a block that holds a stored block
    holds_stored = census_of("gzip", name)["count:stored"] > 0
    rc, out, lanes = _inflate_with(blocks, 0)
    assert rc == 0 and out == text and lanes == (1 if holds_stored else 0), (rc, lanes, holds_stored)
    rc, out, lanes = _inflate_with(blocks, 1)
    assert rc == 0 and out == text and lanes >= 1, (rc, lanes)


def refused(push, blob):
    c = case()
    s = Slimm.for_workload(c["w"], device=0, grouped=True)
    s.set_reference_names(c["w"].ref_names)
    with pytest.raises(Exception) as e:
        push(s, blob)
    s.close()
    return str(e.value)


@pytest.mark.parametrize("name", bzip2_directed.INVALID_NAMES)
def test_invalid_bzip2_variants_are_refused_in_their_words(monkeypatch, name):
    forced(monkeypatch, None)
    blob, words = case()["bad_bzip2"][name]
    msg = refused(lambda s, b: s.push_bzip2_sam_bytes(b, skip=0), blob)
    assert "bzip2-compressed input is not supported unless it decodes" in msg and words in msg, msg
    if name != "combined_crc":   # (a block's error names the byte the block starts at)
        assert re.search(r"block at byte \d+: " + re.escape(words), msg), msg


@pytest.mark.parametrize("name", deflate_directed.INVALID_NAMES)
def test_invalid_gzip_variants_are_refused_in_their_words(monkeypatch, name):
    forced(monkeypatch, None)
    blob, words = case()["bad_gzip"][name]
    msg = refused(lambda s, b: s.push_gzip_sam_bytes(b, skip=0), blob)
    assert "corrupt gzip stream (" + words in msg, msg
