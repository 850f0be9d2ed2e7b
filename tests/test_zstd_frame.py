"""CPU tests of the zstd format code (slimm_amd/csrc/zstd_frame.h) through the host decoder (host/zstd.cpp), built as the
stand-alone program tests/native/san_zstd.cpp under AddressSanitizer and UBSan: the decoder against ZSTD_decompress on the
inputs of tests/sam_zst.py, XXH64 against known answers, the predefined tables through the windowLog-10 input, and the
committed inputs of tests/golden/zstd against the texts made again from their seeds.  Damaged copies -- truncated at every
structural place, a bit flipped anywhere -- end in an error, never in a sanitizer report.  No GPU is touched."""
import os
import random
import subprocess

import pytest

from tests import sam_zst as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_libzstd = pytest.mark.skipif(Z.LIB is None, reason="no libzstd on this machine")


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "san_zstd")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_zstd.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", "zstd.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("texts")
    return {(g, n): Z.case_text(d, g, n) for g in (True, False) for n in (3_000, 400)}


def decode(san, tmp_path, blob):
    p, out = str(tmp_path / "in.zst"), str(tmp_path / "out.bin")
    open(p, "wb").write(blob)
    r = subprocess.run([san, "--out", out, p], capture_output=True, text=True)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return (open(out, "rb").read(), "") if r.returncode == 0 else (None, r.stderr.strip())


def golden_files():
    return [(g, n, f"{'config1' if n == 3_000 else 'short'}_{'grouped' if g else 'any'}_{tag}.sam.zst")
            for g in (True, False) for n, tag in ((3_000, "l3"), (3_000, "l19"), (400, "wlog10"))]


def test_the_inputs_hold_what_they_are_named_for(texts):
    """Level 3: a few blocks of up to 128 KiB, every table FSE-described (mode byte 0xA8), Huffman literals with a tree and
    treeless; level 19 repeats a table; windowLog 10: more than 50 blocks of 1 KiB, almost all treeless, predefined tables,
    a raw literals section.  The Python-written frames: raw blocks only, RLE blocks, frames and a skippable one."""
    for g in (True, False):
        tag = "grouped" if g else "any"
        c = Z.census(Z.golden(f"config1_{tag}_l3.sam.zst"))
        assert c["compressed"] >= 3 and c["mode_bytes"] == {0xA8} and c["lit_huffman"] >= 1 and c["lit_treeless"] >= 1, c
        c = Z.census(Z.golden(f"config1_{tag}_l19.sam.zst"))
        assert c["repeated"] >= 1 and c["fse_tables"] >= 3, c
        c = Z.census(Z.golden(f"short_{tag}_wlog10.sam.zst"))
        assert c["compressed"] >= 50 and c["predefined"] >= 100 and c["lit_treeless"] >= 40 and c["lit_raw"] >= 1, c
        assert Z.walk(Z.golden(f"short_{tag}_wlog10.sam.zst"))[0]["window"] == 1024
    w = Z.written_copies(texts[(True, 3_000)])
    c = Z.census(w["raw_blocks"])
    assert c["raw"] >= 7 and c["rle"] == c["compressed"] == 0, c
    assert Z.census(w["rle_blocks"])["rle"] >= 1
    c = Z.census(w["frames"])
    assert (c["frames"], c["skippable"]) == (4, 1) and c["rle"] >= 1, c
    assert Z.walk(w["frames"])[1]["content_size"] == 0   # (an empty frame)
    assert Z.walk(w["plain_header"])[0]["content_size"] is None and Z.walk(w["plain_header"])[0]["checksum_at"] is None
    assert Z.walk(w["single_segment"])[0]["window"] is None
    assert Z.census(w["skippable_first"])["skippable"] == 1 and Z.walk(w["skippable_first"])[0]["skippable"]


def test_the_committed_inputs_are_the_texts_of_their_seeds(san, tmp_path, texts):
    """... by the host decoder, and by ZSTD_decompress where the machine has libzstd."""
    total = 0
    for g, n, name in golden_files():
        blob = Z.golden(name)
        total += len(blob)
        got, err = decode(san, tmp_path, blob)
        assert got == texts[(g, n)], (name, err)
        if Z.LIB is not None:
            assert Z.decompress(blob, len(texts[(g, n)]) + 1) == texts[(g, n)], name
    assert total < (1 << 20)


def test_the_written_frames_decode_to_their_text(san, tmp_path, texts):
    text = texts[(False, 3_000)]
    for kind, blob in Z.written_copies(text).items():
        got, err = decode(san, tmp_path, blob)
        assert got == text, (kind, err)
        if Z.LIB is not None and kind != "frames":   # (ZSTD_decompress 1.4.8 passes over skippable frames in front only)
            assert Z.decompress(blob, len(text) + 1) == text, kind
    blob, crafted = Z.run_frame(text[:70_000], 100_000, text[70_000:90_000])
    got, err = decode(san, tmp_path, blob)
    assert got == crafted, err
    if Z.LIB is not None:
        assert Z.decompress(blob, len(crafted) + 1) == crafted


@needs_libzstd
@pytest.mark.parametrize("level,window_log", [(1, 0), (3, 0), (9, 0), (19, 0), (3, 10), (19, 10), (3, 12), (-5, 0)])
def test_the_host_decoder_against_libzstd(san, tmp_path, texts, level, window_log):
    """Frames of the machine's libzstd at several levels and windows, with and without content size and checksum, two of
    them back to back: the host decoder gives what ZSTD_decompress gives."""
    text = texts[(True, 3_000)]
    rng = random.Random(level * 31 + window_log)
    noise = bytes(rng.randrange(256) for _ in range(5_000)) + b"A" * 3_000 + text[:20_000] + bytes(200_000)
    for body in (text, noise, b"", b"x"):
        for cs, ck in ((True, True), (False, False)):
            blob = Z.compress(body, level, window_log, cs, ck)
            assert Z.decompress(blob, len(body) + 1) == body
            got, err = decode(san, tmp_path, blob)
            assert got == body, (len(body), cs, ck, err)
    two = Z.compress(text[:100_000], level, window_log) + Z.compress(text[100_000:], level, window_log, False, True)
    got, err = decode(san, tmp_path, two)
    assert got == text, err


def test_xxh64_against_known_answers(san, tmp_path):
    known = {b"": "ef46db3751d8e999", b"a": "d24ec4f1a98c6e5b", b"abc": "44bc2cf5ad770999"}
    rng = random.Random(5)
    data = {k: v for k, v in known.items()}
    for n in (4, 7, 8, 31, 32, 33, 63, 64, 100, 1_000, 4_097):
        b = bytes(rng.randrange(256) for _ in range(n))
        data[b] = "%016x" % Z.xxh64(b)
    for k, v in known.items():
        assert "%016x" % Z.xxh64(k) == v
    for b, want in data.items():
        p = str(tmp_path / "x.bin")
        open(p, "wb").write(b)
        for piece in (1, 5, 32, 50, 1 << 20):
            r = subprocess.run([san, "--xxh64", str(piece), p], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.strip() == want and not r.stderr, (len(b), piece, r.stdout, r.stderr[-500:])


def test_damaged_copies_end_in_an_error_never_in_a_sanitizer_report(san, tmp_path, texts):
    """Every committed input and a written one, truncated at every structural place (and one byte to either side) and with
    one bit flipped at 150 random places: an error with a cause, or -- a flip the checks cannot see -- some text."""
    rng = random.Random(11)
    files, n = [], 0
    for blob in [Z.golden(name) for _, _, name in golden_files()[:3]] + [Z.written_copies(texts[(True, 400)])["frames"]]:
        cuts = set()
        for f in Z.walk(blob):
            cuts.update((f["at"] + 2, f["at"] + 5))
            if f.get("checksum_at"):
                cuts.update((f["checksum_at"], f["checksum_at"] + 2))
            for b in f["blocks"][:40]:
                cuts.update((b["at"], b["at"] + 1, b["at"] + 3, b["at"] + 3 + b["size"] // 2))
                cuts.update(b[k] + d for k in ("huf_at", "fse_at", "bits_at") if b.get(k) for d in (0, 1))
        for c in sorted(c for c in cuts if 0 < c < len(blob)):
            files.append((blob[:c], True))
        for _ in range(150):
            at = rng.randrange(len(blob))
            files.append((blob[:at] + bytes([blob[at] ^ (1 << rng.randrange(8))]) + blob[at + 1:], False))
    paths = []
    for data, _ in files:
        p = str(tmp_path / f"d{n}.zst")
        open(p, "wb").write(data)
        paths.append(p)
        n += 1
    r = subprocess.run([san] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    rows = [l.split("\t") for l in r.stdout.splitlines()]
    assert len(rows) == len(files)
    for row, (_, truncated) in zip(rows, files):
        assert row[1] in ("ok", "error")
        if truncated:
            assert row[1] == "error" and "truncated" in row[2], row
    assert sum(1 for row in rows if row[1] == "error") > len(rows) // 2
