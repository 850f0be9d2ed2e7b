"""The device decoders on a text that looks like a SAM file, on a real MI355X.  Every other `-m gpu` test of compressed input
decodes tests/bam_io.write_sam's text -- SEQ = AAA..., QUAL = *, no tags --, which every compressor turns into long matches:
the decoders' literal paths (LZMA's literal and matched-literal coders, zstd's Huffman streams, deflate trees with long
codes, bzip2 blocks of many selectors) saw a handful of ASCII bytes per line and never a byte >= 0x80.  Here the text is
tests/sam_lifelike.lifelike_text -- random bases, Phred-like qualities, CIGARs, tags, optionally bytes of 128 .. 255 -- of
config1's records (seed 31, 1 000 records: about 380 kB, the smallest text whose xz block holds more than three LZMA chunks),
pushed through all six forms under the settings and cuts of the codec tests.  Every input must give the record count, the
integers of slimm_push_sam_bytes on the plain lifelike text, the CPU oracle's profile, and stats equal to the census of the
tests' own walkers.  test_the_inputs_hold_what_they_are_named_for (no GPU) holds the premise: these inputs compress less than
3.5-fold where write_sam's text compresses more than 10-fold.  No randomly damaged input runs here: damage belongs to
tests/test_device_decoders_sanitized.py, on the CPU."""
import random

import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from tests import sam_deflate as D
from tests import sam_lifelike as L
from tests import sam_xz as X
from tests import sam_zst as Z
from tests.helpers import assert_matches_oracle
from tests.sam_gz import bgzf, header_len

gpu = pytest.mark.gpu
SEED, RECORDS = 31, 1_000
CUTS = [("one", False), ("random", True), ("60k", False)]   # (the cut, whether the codec's *_round=1 knob is set)
XZ_KINDS = ["preset6", "lc4_dict4k", "lc0lp4pb4", "none", "three_streams"]
GZIP_KINDS = ["level6", "mem1", "huffman", "rle", "fixed", "two_members"]
BZIP2_KINDS = ["level1", "level9", "two_streams"]
# (kind, hi_bytes): every kind on the ASCII text, one kind per codec also with bytes of 128 .. 255
XZ_CASES = [(k, False) for k in XZ_KINDS] + [("preset6", True), ("lc0lp4pb4", True)]
GZIP_CASES = [(k, False) for k in GZIP_KINDS] + [("level6", True)]
BZIP2_CASES = [(k, False) for k in BZIP2_KINDS] + [("level9", True)]


def integers(s):
    from tests.test_gpu_compressed_sam import integers as f
    return f(s)


def profile_of(w, grouped, push):
    from tests.test_gpu_compressed_sam import profile_of as f
    return f(w, grouped, push)


def forced(monkeypatch, *values):
    value = ",".join(v for v in values if v)
    if value:
        monkeypatch.setenv("SLIMM_FORCE", value)
    else:
        monkeypatch.delenv("SLIMM_FORCE", raising=False)


def random_cuts(n, seed, lo, hi):
    rng, p, out = random.Random(seed), 0, []
    while True:
        p += rng.randint(lo, hi)
        if p >= n:
            return out
        out.append(p)


def cuts_of(blob, cut):
    return {"one": [], "random": random_cuts(len(blob), 7, 1, 9_000), "60k": list(range(60_000, len(blob), 60_000))}[cut]


_texts, _cases, _blobs = {}, {}, {}


def text_of(grouped, hi, n_records=RECORDS):
    """(the workload, its lifelike text, the header's length): made once."""
    key = (grouped, hi, n_records)
    if key not in _texts:
        w = X.case_workload(grouped, n_records)
        text = L.lifelike_text(w, SEED, hi_bytes=hi)
        _texts[key] = (w, text, header_len(text))
    return _texts[key]


def case(grouped, hi, n_records=RECORDS):
    """... with the oracle's run and the profile of the plain text on the device: made once, shared, never changed."""
    key = (grouped, hi, n_records)
    if key not in _cases:
        w, text, skip = text_of(grouped, hi, n_records)
        s, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        _cases[key] = (w, text, skip, run_workload(w, use_qnames=True), want)
    return _cases[key]


def blobs_of(codec, grouped, hi):
    key = (codec, grouped, hi)
    if key not in _blobs:
        text = text_of(grouped, hi)[1]
        _blobs[key] = {"xz": L.xz_copies, "gzip": L.gzip_copies, "bzip2": L.bzip2_copies}[codec](text)
    return _blobs[key]


_gzip_census = {}


def gzip_census(grouped, hi, kind):
    """Members and deflate blocks by type, by the tests' own walker of deflate blocks (slow: once per input)."""
    key = (grouped, hi, kind)
    if key not in _gzip_census:
        members = blobs_of("gzip", grouped, hi)[kind]
        types = [D.count_types(D.member_blocks(m)) for m in members]
        _gzip_census[key] = {"members": len(members), "stored_blocks": sum(t[0] for t in types), "fixed_blocks": sum(t[1] for t in types),
                             "dynamic_blocks": sum(t[2] for t in types)}
    return _gzip_census[key]


def ratio(text, blob):
    return len(text) / len(blob)


def test_the_inputs_hold_what_they_are_named_for():
    """No GPU.  Every input made from the lifelike text compresses less than 3.5-fold -- it is mostly literals --, and the same
    setting on write_sam's text of the same records more than 10-fold (Z_HUFFMAN_ONLY and Z_RLE, which search for no match
    and cannot reach that on any text: more than twice as well as on the lifelike text); the xz inputs hold the chunks, properties and checks
    they are named for, and the level-6 and memLevel-1 gzip members the dynamic blocks the device tests ask for."""
    w, text, _ = text_of(True, False)
    hi_text = text_of(True, True)[1]
    plain = L.plain_text(w)
    assert max(hi_text) >= 0xf0 and max(text) < 0x80
    copies = lambda t: {**{("xz", k): v for k, v in L.xz_copies(t).items()}, **{("gzip", k): b"".join(v) for k, v in L.gzip_copies(t).items()},
                        **{("bzip2", k): v for k, v in L.bzip2_copies(t).items()}, ("bgzf", "blocks"): bgzf(t, seed=3, lo=500, hi=65_000)}
    lifelike, hi_copies, easy = copies(text), copies(hi_text), copies(plain)
    for key in lifelike:
        assert 1.2 < ratio(text, lifelike[key]) < 3.5, (key, ratio(text, lifelike[key]))
        assert 1.2 < ratio(hi_text, hi_copies[key]) < 3.5, (key, ratio(hi_text, hi_copies[key]))
        if key in (("gzip", "huffman"), ("gzip", "rle")):   # (these two strategies search for no match: at most 8-fold on any text)
            assert ratio(plain, easy[key]) > 2 * ratio(text, lifelike[key]), (key, ratio(plain, easy[key]))
        else:
            assert ratio(plain, easy[key]) > 10, (key, ratio(plain, easy[key]))
    bam, skip, body = L.lifelike_bam(w, SEED)
    assert ratio(body, bam) < 3.5
    # xz: what the device tests assert of the stats, by the walker
    for kind, blob in ((k, lifelike[("xz", k)]) for k in XZ_KINDS):
        c = X.census(blob)
        assert c["lzma_chunks"] >= 3 and c["lzma_chunks"] > c["state_resets"], (kind, c)
        assert c["odd_props"] == (1 if kind in ("lc4_dict4k", "lc0lp4pb4") else 0), (kind, c)
        assert c["streams"] == (3 if kind == "three_streams" else 1)
        assert (c["check_none"], c["check_crc32"]) == (int(kind == "none"), int(kind == "lc4_dict4k")), (kind, c)
    assert gzip_census(True, False, "level6")["dynamic_blocks"] >= 9
    assert gzip_census(True, False, "mem1")["dynamic_blocks"] >= 1_000


def check(s, got, want, o):
    assert got == want
    assert_matches_oracle(s, o)


@gpu
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind,hi", XZ_CASES)
@pytest.mark.parametrize("cut,round1", CUTS)
def test_xz(monkeypatch, grouped, kind, hi, cut, round1):
    w, text, skip, o, want = case(grouped, hi)
    blob = blobs_of("xz", grouped, hi)[kind]
    forced(monkeypatch, "xz_round=1" if round1 else "")
    s, got = profile_of(w, grouped, lambda s: s.push_xz_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    st = s.xz_stats()
    check(s, got, want, o)
    from tests.test_gpu_xz_sam import assert_census
    assert_census(st, blob)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob), st
    assert st["lzma_chunks"] >= 3 and st["lzma_chunks"] > st["state_resets"], st
    if kind == "preset6":
        assert st["max_dist"] > 65_536, st
    if kind == "lc4_dict4k":
        assert st["max_dist"] <= 4_096, st
    if kind in ("lc4_dict4k", "lc0lp4pb4"):
        assert st["odd_props"] >= 1, st
    s.close()


@gpu
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind,hi", GZIP_CASES)
@pytest.mark.parametrize("chunk", ["gzip_chunk=2048", ""])
@pytest.mark.parametrize("cut,round1", CUTS)
def test_gzip(monkeypatch, grouped, kind, hi, chunk, cut, round1):
    """A chunk start every 2 048 compressed bytes, and the default chunk of 64 KiB.  resolved_bytes counts what a chunk copies
    from the chunk in front of it: it is asked for, under both chunk sizes, where the stream has copies and more than one
    chunk -- level 6, level 1 and the two members, each member of more than 100 kB and so of several 64 KiB chunks.
    Huffman-only has no copy, Z_RLE none farther than one byte, and fixed blocks start no chunk."""
    w, text, skip, o, want = case(grouped, hi)
    blob = b"".join(blobs_of("gzip", grouped, hi)[kind])
    forced(monkeypatch, chunk, "gzip_round=1" if round1 else "")
    s, got = profile_of(w, grouped, lambda s: s.push_gzip_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    st = s.gzip_stats()
    check(s, got, want, o)
    census = gzip_census(grouped, hi, kind)
    assert {k: st[k] for k in census} == census, (st, census)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob), st
    assert st["dropped"] == 0 and st["forced_starts"] == 0, st
    if kind == "level6":
        assert st["dynamic_blocks"] >= 9, st
    if kind == "mem1" and chunk:
        assert st["dynamic_blocks"] >= 1_000 and st["chunks"] >= 100, st
    if kind in ("level6", "mem1", "two_members"):
        assert st["chunks"] > 1 and st["resolved_bytes"] > 0, st
    s.close()


@gpu
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("kind,hi", BZIP2_CASES)
@pytest.mark.parametrize("cut,round1", CUTS)
def test_bzip2(monkeypatch, grouped, kind, hi, cut, round1):
    w, text, skip, o, want = case(grouped, hi)
    blob = blobs_of("bzip2", grouped, hi)[kind]
    forced(monkeypatch, "bzip2_round=1" if round1 else "")
    s, got = profile_of(w, grouped, lambda s: s.push_bzip2_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    check(s, got, want, o)
    s.close()


@gpu
@pytest.mark.parametrize("kind", sorted(L.ZSTD_KINDS))
@pytest.mark.parametrize("cut,round1", CUTS)
def test_zstd(monkeypatch, kind, cut, round1):
    """The committed files of tests/golden/zstd_lifelike (300 records, grouped): no test here depends on the machine's libzstd."""
    hi = L.ZSTD_KINDS[kind][1]
    w, text, skip, o, want = case(True, hi, L.ZSTD_RECORDS)
    blob = L.zstd_golden(kind)
    forced(monkeypatch, "zstd_round=1" if round1 else "")
    s, got = profile_of(w, True, lambda s: s.push_zstd_sam_bytes(blob, skip=skip, cuts=cuts_of(blob, cut)))
    st = s.zstd_stats()
    check(s, got, want, o)
    census = Z.census(blob)
    assert st["text_bytes"] == len(text) and st["compressed_bytes"] == len(blob), st
    assert (st["frames"], st["skippable"]) == (census["frames"], census["skippable"]), (st, census)
    assert (st["raw_blocks"], st["rle_blocks"], st["compressed_blocks"]) == (census["raw"], census["rle"], census["compressed"]), (st, census)
    assert (st["huffman_trees"], st["treeless"], st["plain_literals"]) == (census["lit_huffman"], census["lit_treeless"], census["lit_raw"] + census["lit_rle"]), (st, census)
    assert (st["predefined"], st["rle_tables"], st["fse_tables"], st["repeated"]) == (census["predefined"], census["rle_tables"], census["fse_tables"], census["repeated"]), (st, census)
    assert st["huffman_trees"] >= 1 and st["fse_tables"] >= 3 and st["sequences"] > 1_000, st
    assert st["checksums"] == (1 if L.ZSTD_KINDS[kind][4] else 0), st
    s.close()


@gpu
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("hi", [False, True])
@pytest.mark.parametrize("window", [0, 60_000])
def test_bgzf_sam(grouped, hi, window):
    """BGZF blocks of 500 .. 65 000 bytes of the text, cut inside lines; whole, and in windows of 60 000 compressed bytes."""
    w, text, skip, o, want = case(grouped, hi)
    blob = bgzf(text, seed=SEED, lo=500, hi=65_000)
    s, got = profile_of(w, grouped, lambda s: s.push_bgzf_sam_blocks(blob, skip=skip, window=window))
    check(s, got, want, o)
    s.close()


@gpu
@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("window", [0, 60_000])
def test_bgzf_bam(grouped, window):
    """A BGZF BAM of the same records with random packed bases, quality bytes 0 .. 93 and lengths 0 .. 300
    (bam_record_bytes(lifelike_seed=)) against slimm_push_records of the workload's arrays."""
    w = text_of(grouped, False)[0]
    o = run_workload(w, use_qnames=True)
    blob, skip, _ = L.lifelike_bam(w, SEED)
    s1 = Slimm.for_workload(w, device=0, grouped=grouped)
    s1.push_records(w.records)
    s1.get_profiles()
    want = integers(s1)
    s1.close()
    s, got = profile_of(w, grouped, lambda s: s.push_bgzf_blocks(blob, skip=skip, window=window))
    check(s, got, want, o)
    s.close()
