"""lz4-compressed SAM on a real MI355X: slimm_push_lz4_sam_bytes (the file's bytes, cut anywhere; frames and blocks walked on
the host, the blocks' tokens walked a wave per block through an LDS ring, the text built in parallel over its bytes and
resolved by pointer doubling, the text found and decoded as SAM) against slimm_push_sam_bytes on the same text and the CPU
oracle.  slimm_get_lz4_stats says that an input reached what it was built for.  The inputs: tests/sam_lz4.py -- the committed
compressor-made files of tests/golden/lz4, frames written in Python, and the directed inputs, each of which states a content
checksum that the decoder verifies (which is what turns one wrong byte of the text into a failure); liblz4 is not needed.
SLIMM_FORCE keys named here: lz4_round=N (decoded every N compressed bytes: frame headers, block headers, blocks and checksums
cut across rounds), lz4_round_text=N (a round's text at most: a round a block, linked copies reach into the history of an
earlier round).  The staging input (sam_lz4.staging_frame) is made for the kernel's chunk of 2 048 bytes (kLz4Chunk): 4 097
blocks put its long-extension sequence behind k = 0 .. 4 096 literal bytes, two chunks' worth."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from oracle.binding import run_workload
from slimm_amd.profiler import Slimm
from tests import sam_lz4 as L
from tests.helpers import assert_matches_oracle
from tests.test_gpu_compressed_sam import integers, profile_of

pytestmark = pytest.mark.gpu

SLIMM_OK, SLIMM_E_INVALID = 0, -1   # (include/slimm_hip.h)
WORDS = "lz4-compressed input is not supported unless it decodes: "
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "slimm_amd", "slimm")
GOLDEN = ["b4", "linked9", "default", "short"]
WRITTEN = ["stored_blocks", "packed_independent", "packed_linked", "linked_mixed", "frames"]
EMU = os.environ.get("SLIMM_EMU") == "1"


def forced(monkeypatch, value):
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


_shared = {}


def case(grouped, n_records=3_000, tail_newline=True):
    """The text, its header's length, the oracle's run and the profile of the plain text: made once."""
    key = (grouped, n_records, tail_newline)
    if key not in _shared:
        w = L.case_workload(grouped, n_records)
        with tempfile.TemporaryDirectory() as d:
            text = L.case_text(d, grouped, n_records)
        text = text if tail_newline else text[:-1]
        skip = L.header_len(text)
        s, want = profile_of(w, grouped, lambda s: s.push_sam_bytes(text[skip:]))
        s.close()
        _shared[key] = (w, text, skip, run_workload(w, use_qnames=True), want)
    return _shared[key]


def blob_of(grouped, kind):
    """(the case, the lz4 bytes) of an input kind."""
    tag = "grouped" if grouped else "any"
    if kind in GOLDEN:
        if kind == "short":
            return case(True, 400), L.golden("short_grouped_b4.sam.lz4")
        return case(grouped), L.golden(f"config1_{tag}_{kind}.sam.lz4")
    c = case(grouped)
    if ("written", grouped) not in _shared:
        _shared[("written", grouped)] = L.written_copies(c[1])
    return c, _shared[("written", grouped)][kind]


def directed():
    """The 50-record case and the directed inputs on its text: made once."""
    if "directed" not in _shared:
        c = case(True, 50)
        _shared["directed"] = (c, L.INPUTS(c[1][:c[2]], c[1][c[2]:]), L.INVALID(c[1][:c[2]], c[1][c[2]:]))
    return _shared["directed"]


def assert_census(st, blob, text_len):
    census = L.census(blob)
    assert st["text_bytes"] == text_len and st["compressed_bytes"] == len(blob), st
    assert (st["frames"], st["skippable"], st["linked"]) == (census["frames"], census["skippable"], census["linked"]), (st, census)
    assert (st["stored_blocks"], st["compressed_blocks"], st["sequences"]) == (census["stored"], census["compressed"], census["sequences"]), (st, census)
    assert (st["block_checksums"], st["content_checksums"]) == (census["block_sums"], census["content_sums"]), (st, census)


CUTS = [("one", ""), ("random", "lz4_round=1"), ("block", "lz4_round_text=65536")]


@pytest.mark.parametrize("grouped,kind", [(g, k) for g in (True, False) for k in GOLDEN + WRITTEN if g or k != "short"])   # (the 400-record text: grouped only)
@pytest.mark.parametrize("cut,force", CUTS)
def test_lz4_sam_bytes_give_the_partials_of_the_text(monkeypatch, grouped, kind, cut, force):
    """The file's bytes pushed whole, cut at random offsets (inside frame headers, block headers, blocks and checksums; with
    lz4_round=1 every push is decoded as far as it goes and the rest waits for the next push), and with a round per block."""
    (w, text, skip, o, want), blob = blob_of(grouped, kind)
    cuts = random_cuts(len(blob), 7, 1, 9_000) if cut == "random" else []
    forced(monkeypatch, force)
    s, got = profile_of(w, grouped, lambda s: s.push_lz4_sam_bytes(blob, skip=skip, cuts=cuts))
    st = s.lz4_stats()
    assert got == want
    assert_matches_oracle(s, o)
    assert_census(st, blob, len(text))
    if kind == "b4":
        assert st["compressed_blocks"] == 7 and st["linked"] == 0 and st["front_bytes"] == 0, st
    if kind == "linked9":
        assert st["linked"] == 1 and st["block_checksums"] == 7 and st["front_bytes"] > 0, st
        if cut == "block":   # (a round a block: what a block copies from the blocks in front comes from the history kept on the device)
            assert st["rounds"] == 7 and st["history_bytes"] == st["front_bytes"] > 0, st
    if kind == "default":
        assert st["compressed_blocks"] == 1 and st["content_checksums"] == 1, st
    if kind in ("packed_linked", "linked_mixed") and cut == "block":
        assert st["rounds"] > 3 and st["history_bytes"] > 0, st
    if kind == "frames":
        assert st["frames"] == 5 and st["skippable"] == 2, st
    if cut == "random" and st["stored_blocks"] + st["compressed_blocks"] > 1 and len(blob) > 20_000:
        assert st["rounds"] > 1, st
    s.close()


def _directed_names():
    return ["stored_only", "linked_mixed", "reach_65535", "first_byte", "lengths", "offsets_1_2_3", "sequence_counts", "zero_literals_last",
            "staging"] + ["flags_%d" % k for k in range(8)] + ["empty_first", "frames"]


@pytest.mark.parametrize("name", _directed_names())
@pytest.mark.parametrize("cut,force", CUTS)
def test_directed_inputs_give_the_partials_of_the_text(monkeypatch, name, cut, force):
    """Every directed good input whole, cut at random offsets with a round per push, and with a round per block; its content
    checksums hold, so every byte of the directed structures was decoded as the Python decoder decodes it."""
    (w, _, _, o, want), inputs, _ = directed()
    assert sorted(inputs) == sorted(_directed_names())
    blob, text, skip = inputs[name]
    cuts = random_cuts(len(blob), 7, 1, max(9_000, len(blob) // 20)) if cut == "random" else []
    forced(monkeypatch, force)
    s, got = profile_of(w, True, lambda s: s.push_lz4_sam_bytes(blob, skip=skip, cuts=cuts))
    st = s.lz4_stats()
    assert got == want
    assert_matches_oracle(s, o)
    assert_census(st, blob, len(text))
    if name == "reach_65535" and cut == "block":
        assert st["history_bytes"] >= 40, st
    if name == "staging":
        assert st["compressed_blocks"] >= 4_097, st
    s.close()


@pytest.mark.parametrize("force", ["", "lz4_round=1"])
def test_last_line_without_newline(monkeypatch, force):
    """The text's last line has no newline: it is a line all the same -- also when the last push carries no byte."""
    w, text, skip, o, _ = case(True, tail_newline=False)
    forced(monkeypatch, force)
    blob = L.Frame(linked=True).stored(text[:40_000]).packed(text[40_000:]).bytes(block_sums=True)
    for empty_last in (False, True):
        s, _ = profile_of(w, True, lambda s: s.push_lz4_sam_bytes(blob, skip=skip, window=5_000, empty_last=empty_last))
        assert_matches_oracle(s, o)
        s.close()


def profile_of_any(w, push):
    s = Slimm.for_workload(w, device=0, grouped=False)
    s.set_reference_names(w.ref_names)
    n = push(s)
    s.get_profiles()
    return s, (n, integers(s))


@pytest.mark.parametrize("run,block_id", [(100_000, 5), ((4 << 20) - 600, 7)])
def test_a_long_run_at_offset_1_resolves_within_the_bound(monkeypatch, run, block_id):
    """One match of 100 000 bytes, and one block of 4 MiB of text, at offset 1 -- the chain of copies is as long as the run --,
    in a SEQ field: pointer doubling resolves it in at most ceil(log2(text + history)) + 1 passes."""
    if EMU and run > 100_000:
        pytest.skip("4 MiB of text: too slow a lane at a time")
    w, text, skip, _, _ = case(False)
    lines = text[skip:].split(b"\n")
    f = lines[0].split(b"\t")
    f[5], f[9], f[10] = b"%dM" % (run + 1), b"A", b"*"
    front = b"\n".join(lines[1:4]) + b"\n" + b"\t".join(f[:10])
    back = b"\t" + b"\t".join(f[10:]) + b"\n"
    rest = b"\n".join(lines[4:40]) + b"\n"
    fr = L.Frame(linked=True, block_id=block_id).compressed([(front, 1, run)], back).packed(rest)
    crafted = bytes(fr.out)
    assert crafted.count(b"A" * (run + 1)) == 1 and len(front) + run + len(back) <= 1 << (8 + 2 * block_id)
    blob = fr.bytes(content_size=True)
    forced(monkeypatch, "")
    s1, want = profile_of_any(w, lambda s: s.push_sam_bytes(crafted))
    s2, got = profile_of_any(w, lambda s: s.push_lz4_sam_bytes(blob))
    st = s2.lz4_stats()
    assert got == want
    bound = (len(crafted) - 1).bit_length() + 1
    assert 1 <= st["passes"] <= bound, (st, bound)
    assert st["content_checksums"] == 1 and st["text_bytes"] == len(crafted), st
    s1.close()
    s2.close()


def push_error(w, blob, skip, **kw):
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception) as e:
        s.push_lz4_sam_bytes(blob, skip=skip, **kw)
    s.close()
    return str(e.value)


def host_words(tmp_path, name, data):
    """What `slimm --host-decode`'s reader says of the same bytes: the words behind the path-free part of its message."""
    q = str(tmp_path / f"{name}.sam.lz4")
    open(q, "wb").write(data)
    r = subprocess.run([CLI, "--dump-raw", q], capture_output=True)
    assert r.returncode != 0 and WORDS.encode() in r.stderr, (name, r.stderr[-300:])
    msg = r.stderr.decode()
    return msg[msg.index(WORDS):msg.rindex(": " + q)]


def flipped(blob, at, bit=0x10):
    b = bytearray(blob)
    b[at] ^= bit
    return bytes(b)


def damaged(text, blob):
    """{name: (bytes, a word of the cause)}: damaged copies of the linked fixture, and headers the reader does not take."""
    fr = L.walk(blob)[0]
    blocks = fr["blocks"]
    plain = L.Frame().stored(text)
    big = L.frame_header(block_id=4) + (70_000).to_bytes(4, "little") + bytes(70_000) + bytes(4)
    return {
        "header_checksum": (flipped(blob, fr["hc_at"]), "header checksum mismatch"),
        "block_checksum": (flipped(blob, blocks[3]["sum_at"]), "block checksum mismatch"),
        "block_byte": (flipped(blob, blocks[2]["at"] + 100), "block checksum mismatch"),
        "content_checksum": (plain.bytes(wrong_sum=True), "content checksum mismatch"),
        "content_size": (plain.bytes(wrong_size=True), "content size mismatch"),
        "block_over_maximum": (big, "a block larger than its maximum"),
        "reserved_flg": (L.frame_header(reserved=1) + bytes(4), "a reserved bit is set"),
        "reserved_bd": (L.frame_header(bd_reserved=1) + bytes(4), "a reserved bit is set"),
        "version_0": (L.frame_header(version=0) + bytes(4), "a frame version other than 1"),
        "dictionary": (L.frame_header(dict_id=5) + bytes(4), "a dictionary"),
        "legacy": (L.LEGACY + blob[4:], "the legacy lz4 format"),
        "junk": (blob + b"junk!", "start no frame"),
        "two_thirds": (blob[:2 * len(blob) // 3], "truncated"),
        "inside_frame_header": (blob[:9], "truncated"),
        "inside_block_header": (blob[:blocks[1]["at"] + 2], "truncated"),
        "inside_block_checksum": (blob[:blocks[1]["sum_at"] + 1], "truncated"),
        "no_end_mark": (blob[:fr["end_at"]], "truncated"),
        "inside_end_mark": (blob[:fr["end_at"] + 3], "truncated"),
        "inside_content_checksum": (plain.bytes()[:-2], "truncated"),
        "no_content_checksum": (plain.bytes()[:-4], "truncated"),
        "second_frame_magic": (blob + blob[:2], "truncated"),
    }


def test_errors_are_the_host_readers_words_and_the_context_stays_usable(tmp_path, monkeypatch):
    """Every directed error and every damaged copy: SLIMM_E_INVALID in the words of `slimm`'s host reader on the same bytes --
    pushed whole, and in pieces with a round per push (so that a truncated file has waited before it ends).  Damage is met as
    data: nothing faults.  After a failure and a reset the context reads a good file."""
    (w, text, skip, o, want), blob = blob_of(True, "linked9")
    (wd, _, skipd, _, _), _, invalid = directed()
    forced(monkeypatch, "")
    cases = [(name, w, skip, data, word) for name, (data, word) in damaged(text, blob).items()]
    cases += [(name, wd, skipd, data, word) for name, (data, word) in invalid.items()]
    for name, wk, sk, data, word in cases:
        host = host_words(tmp_path, name, data)
        assert word in host, (name, host)
        for kw, force in ((dict(), ""), (dict(cuts=random_cuts(len(data), 3, 1, 3_000)), "lz4_round=1"), (dict(window=3_000, empty_last=True), "lz4_round=1")):
            forced(monkeypatch, force)
            msg = push_error(wk, data, sk, **kw)
            assert host in msg, (name, kw.keys(), msg, host)
    forced(monkeypatch, "")
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    with pytest.raises(Exception):
        s.push_lz4_sam_bytes(flipped(blob, L.walk(blob)[0]["blocks"][4]["sum_at"]), skip=skip)
    s.reset()
    assert s.push_lz4_sam_bytes(blob, skip=skip) == len(w.records)
    s.get_profiles()
    assert integers(s) == want
    assert_matches_oracle(s, o)
    s.close()


def test_blocks_liblz4_refuses_are_taken_as_the_host_reader_takes_them(monkeypatch):
    """Blocks whose last match ends 3 .. 7 bytes in front of the block's end (LZ4_decompress_safe refuses them: DESIGN §9): the
    device decodes them to the text the Python decoder gives -- the content checksum holds -- as the host reader does."""
    (w, text, skip, o, want), _, _ = directed()
    forced(monkeypatch, "")
    for name, (body, comment) in L.UNSAFE_BUT_TAKEN().items():
        f = L.Frame().stored(text[:skip])
        f.blocks.append((False, body))
        f.out += comment
        f.stored(b"\n" + text[skip:])
        s, got = profile_of(w, True, lambda s: s.push_lz4_sam_bytes(f.bytes(), skip=skip + len(comment) + 1))
        assert got == want and s.lz4_stats()["content_checksums"] == 1, name
        s.close()


def test_lz4_does_not_mix_with_other_forms_and_is_not_cut_by_byte_range(monkeypatch):
    (w, text, skip, _, _), blob = blob_of(True, "b4")
    forced(monkeypatch, "")
    got = C.c_uint64()
    filler = np.zeros(64, dtype=np.uint8)
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_bam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 0, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_lz4_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_push_lz4_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), 100, skip, 0, C.byref(got)) == SLIMM_OK
    assert s.L.slimm_push_zstd_sam_bytes(s.ctx, filler.ctypes.data_as(C.c_void_p), 10, 0, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "do not mix" in s.L.slimm_last_error(s.ctx).decode()
    s.close()
    s = Slimm.for_workload(w, device=0, grouped=True)
    s.set_reference_names(w.ref_names)
    assert s.L.slimm_set_input_mid_file(s.ctx, 0, 1) == SLIMM_OK
    assert s.L.slimm_push_lz4_sam_bytes(s.ctx, buf.ctypes.data_as(C.c_void_p), buf.size, skip, 1, C.byref(got)) == SLIMM_E_INVALID
    assert "an lz4 stream is not cut by byte range" in s.L.slimm_last_error(s.ctx).decode()
    s.close()


def test_one_lifelike_text_reads_as_its_plain_text(monkeypatch):
    """A lifelike SAM text (tests/sam_lifelike.py) as a linked frame of the Python writer."""
    from tests.test_gpu_lifelike_sam import case as lifelike_case
    w, text, skip, o, want = lifelike_case(True, True)
    forced(monkeypatch, "lz4_round_text=65536")
    blob = L.Frame(linked=True).packed(text).bytes(block_sums=True, content_size=True)
    s, got = profile_of(w, True, lambda s: s.push_lz4_sam_bytes(blob, skip=skip))
    assert got == want and s.lz4_stats()["history_bytes"] > 0
    assert_matches_oracle(s, o)
    s.close()
