"""The directed xz and zstd inputs (tests/lzma_directed.py, tests/zstd_directed.py: one path family of the entropy decoders each,
shown to reach it by tests/test_codec_paths.py) on a real MI355X: each through slimm_push_xz_sam_bytes /
slimm_push_zstd_sam_bytes whole, and cut at random offsets with a round per push; the history cases (the writers' HISTORY) once more
with a round per block (zstd_round_text=1 / xz_round_text=1), so that repeated offsets and copies cross rounds -- an xz block's
dictionary starts with it, so there the case is a stream of two blocks that must not see each other.  The partials must equal those of slimm_push_sam_bytes on the plain text, the
stats the container census of the tests' walkers, the profile the oracle's.  Every input carries a check the decoder verifies
(CRC32 / CRC64 per xz block, the zstd content checksum), which is what turns one wrong byte of the text into a failure.  The
inputs are small (50 records; 4 and 2 MiB of uncompressed filler in the two far-distance ones, under 8 MiB of text in all): the file also runs on the host
emulator (SLIMM_EMU=1)."""
import tempfile

import pytest

from oracle.binding import run_workload
from tests import lzma_directed, sam_xz as X, sam_zst as Z, zstd_directed
from tests.helpers import assert_matches_oracle
from tests.test_gpu_compressed_sam import profile_of
from tests.test_gpu_xz_sam import assert_census, forced, random_cuts

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
        _shared.update(w=w, want=want, oracle=run_workload(w, use_qnames=True), xz=lzma_directed.INPUTS(text[:skip], text[skip:]),
                       zstd=zstd_directed.INPUTS(text[:skip], text[skip:]))
    return _shared


def cuts_of(blob, cut):
    return random_cuts(len(blob), 7, 1, max(9_000, len(blob) // 20)) if cut == "random" else []


CUTS = [("one", ""), ("random", "{}_round=1")]


def cases(mod, codec):
    """(name, cut, force): every input whole and cut at random offsets; a history case also under its force key."""
    out = [(name, cut, force.format(codec)) for name in mod.NAMES for cut, force in CUTS]
    return out + [(name, "history", None) for name in mod.HISTORY]


@pytest.mark.parametrize("name,cut,force", cases(lzma_directed, "xz"))
def test_directed_xz_inputs_give_the_partials_of_the_text(monkeypatch, name, cut, force):
    c = case()
    blob, text, skip, _, history = c["xz"][name]
    assert (history is not None) == (name in lzma_directed.HISTORY)
    forced(monkeypatch, history if cut == "history" else force)
    s, got = profile_of(c["w"], True, lambda s: s.push_xz_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    st = s.xz_stats()
    assert got == c["want"]
    assert_matches_oracle(s, c["oracle"])
    assert_census(st, blob)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob) and st["max_dist"] <= len(text), st
    if name == "distance_slots":
        assert st["max_dist"] == 1 << 22, st
    if cut == "history":     # (a round a block)
        assert st["rounds"] >= st["blocks"] == 2, st
    s.close()


@pytest.mark.parametrize("name,cut,force", cases(zstd_directed, "zstd"))
def test_directed_zstd_inputs_give_the_partials_of_the_text(monkeypatch, name, cut, force):
    c = case()
    blob, text, skip, _, history = c["zstd"][name]
    assert (history is not None) == (name in zstd_directed.HISTORY)
    forced(monkeypatch, history if cut == "history" else force)
    s, got = profile_of(c["w"], True, lambda s: s.push_zstd_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    st = s.zstd_stats()
    assert got == c["want"]
    assert_matches_oracle(s, c["oracle"])
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob)
    census, frames = Z.census(blob), Z.walk(blob)
    assert st["frames"] == census["frames"] and st["skippable"] == census["skippable"]
    assert (st["raw_blocks"], st["rle_blocks"], st["compressed_blocks"]) == (census["raw"], census["rle"], census["compressed"])
    assert (st["huffman_trees"], st["treeless"]) == (census["lit_huffman"], census["lit_treeless"]), st
    assert (st["predefined"], st["rle_tables"], st["fse_tables"], st["repeated"]) == (census["predefined"], census["rle_tables"], census["fse_tables"],
                                                                                   census["repeated"]), (st, census)
    assert st["sequences"] == sum(b.get("n_seq", 0) for f in frames for b in f["blocks"]), st
    assert st["checksums"] == sum(1 for f in frames if f.get("checksum_at") is not None)
    if cut == "history":     # (a round a block: what a block repeats or copies lies in an earlier round)
        assert st["rounds"] >= sum(len(f["blocks"]) for f in frames) - 1 and st["history_bytes"] > 0, st
    s.close()
