"""CPU tests of the xz format code (slimm_amd/csrc/xz_stream.h: the container, the LZMA2 chunks, the LZMA decoder and the
CRC64 helpers the device decoder runs too) through the host decoder (host/xz.cpp), built as the stand-alone program
tests/native/san_xz.cpp under AddressSanitizer and UBSan: every committed input of tests/golden/xz and every container
written in Python decodes to its text and to the walker's census; the x86-filtered file is refused by name; thousands of
damaged copies end in `ok` or an error line, never in a sanitizer report; the CRC64 combiner agrees with the serial CRC; the
index reader returns the blocks.  No GPU is touched, no `xz` binary and no liblzma is needed."""
import os
import subprocess

import pytest

from tests import sam_xz as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS_REFUSED = "a filter chain other than LZMA2 alone (filter id 4)"
COUNTS = ("streams", "blocks", "lzma_chunks", "raw_chunks", "state_resets", "prop_changes", "odd_props", "check_none", "check_crc32", "check_crc64",
          "sha256_unverified", "text", "index_records")


@pytest.fixture(scope="module")
def san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "san_xz")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_xz.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", "xz.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def texts(tmp_path_factory):
    d = tmp_path_factory.mktemp("texts")
    return {(g, n): X.case_text(d, g, n) for g in (True, False) for n in (3_000, 1_000, 15_000)}


def clean(r):
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r


def inputs(texts, grouped):
    """{kind: (text, xz bytes)}: every committed and every written input."""
    tag = "grouped" if grouped else "any"
    out = {k: (texts[(grouped, n)], X.golden(name.format(tag))) for k, (n, name) in X.GOLDEN_KINDS.items()}
    short = texts[(grouped, 1_000)]
    out.update({k: (short, blob) for k, blob in X.written_copies(short, tag).items()})
    return out


def test_the_inputs_hold_what_they_are_named_for(texts):
    for g in (True, False):
        ins = inputs(texts, g)
        c = {k: X.census(blob) for k, (_, blob) in ins.items()}
        assert c["mt"]["blocks"] >= 8 and all(b["sizes"] != (None, None) for b in X.walk(ins["mt"][1])[0]["blocks"])
        assert c["blocks"]["blocks"] >= 8 and all(b["sizes"] == (None, None) for b in X.walk(ins["blocks"][1])[0]["blocks"])
        controls = [ch["control"] for ch in X.walk(ins["one"][1])[0]["blocks"][0]["chunks"]]
        assert c["one"]["blocks"] == 1 and controls[0] & 0xE0 == 0xE0 and controls[1] & 0xE0 == 0x80, controls
        assert c["lc0lp2"]["odd_props"] == 1 and c["lc0lp2"]["check_crc32"] == 1 and c["lc4"]["odd_props"] == 1
        assert c["none"]["check_none"] == 1 and c["sha256"]["sha256_unverified"] == 1
        assert c["stored_chunks"]["raw_chunks"] > 1 and c["stored_chunks"]["lzma_chunks"] == 0 and c["stored_chunks"]["blocks"] == 2
        assert c["reblocked"]["blocks"] == 3 and c["reblocked"]["odd_props"] == 1 and c["reblocked"]["check_crc32"] == 3
        two = X.walk(ins["two_streams_padded"][1])
        assert [len(s["blocks"]) for s in two] == [1, 2] and [s["padding"] for s in two] == [8, 4] and [s["check"] for s in two] == [4, 1]
        assert [len(s["blocks"]) for s in X.walk(ins["empty_stream"][1])] == [0, 3]


@pytest.mark.parametrize("grouped", [True, False])
def test_every_input_decodes_to_its_text_and_to_the_walkers_census(san, texts, tmp_path, grouped):
    for kind, (text, blob) in inputs(texts, grouped).items():
        p, out = str(tmp_path / f"{kind}.xz"), str(tmp_path / "out.bin")
        open(p, "wb").write(blob)
        r = clean(subprocess.run([san, "--out", out, p], capture_output=True, text=True))
        assert r.returncode == 0, (kind, r.stderr)
        assert open(out, "rb").read() == text, kind
        r = clean(subprocess.run([san, "--counts", p], capture_output=True, text=True))
        got = dict((ln.split("=")[0], int(ln.split("=")[1])) for ln in r.stdout.split())
        want = X.census(blob)
        assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, kind
        assert got["match_bytes"] > 0 or want["lzma_chunks"] == 0
        assert got["max_dist"] <= len(text)
        r = clean(subprocess.run([san, p], capture_output=True, text=True))
        assert r.stdout == f"{p}\tok\t{len(text)}\t{X.crc64(text):016x}\n", kind


def test_python_lzma_agrees_where_it_is_importable(texts):
    lzma = pytest.importorskip("lzma")
    for g in (True, False):
        for kind, (text, blob) in inputs(texts, g).items():
            if kind != "two_streams_padded":   # (lzma.decompress stops at stream padding: it takes what follows for garbage)
                assert lzma.decompress(blob) == text, kind


@pytest.mark.parametrize("grouped", [True, False])
def test_a_filter_chain_other_than_lzma2_is_refused_by_name(san, tmp_path, grouped):
    p = str(tmp_path / "bcj.xz")
    open(p, "wb").write(X.golden(X.REFUSED_KIND[1].format("grouped" if grouped else "any")))
    r = clean(subprocess.run([san, p], capture_output=True, text=True))
    assert r.stdout == f"{p}\terror\tblock header at byte 12: {WORDS_REFUSED}\n"


def test_damage_at_every_structural_place_is_an_error_that_names_it(san, texts, tmp_path):
    text = texts[(True, 1_000)]
    blob = X.written_copies(text, "grouped")["reblocked"]
    s = X.walk(blob)[0]
    b0, b1 = s["blocks"][0], s["blocks"][1]
    ch = b0["chunks"][0]

    def flipped(at, bit=0x10):
        b = bytearray(blob)
        b[at] ^= bit
        return bytes(b)

    def with_byte(at, v):
        b = bytearray(blob)
        b[at] = v
        return bytes(b)

    no_reset = X.stream_of([(X.block_header(), X.raw_chunks(text, 40_000, first_control=2), text)])
    cases = {
        "inside_the_stream_header": (blob[:7], "stream header at byte 0: truncated"),
        "behind_the_stream_header": (blob[:12], "block header at byte 12: truncated"),
        "inside_a_block_header": (blob[:b0["at"] + 3], "block header at byte 12: truncated"),
        "inside_a_chunk_header": (blob[:ch["at"] + 2], "truncated"),
        "inside_a_chunk": (blob[:ch["at"] + 100], "truncated"),
        "behind_the_end_marker": (blob[:b0["pad_at"]], "truncated"),
        "inside_the_check": (blob[:b0["check_at"] + 2], "truncated"),
        "between_blocks": (blob[:b1["at"]], "truncated"),
        "inside_the_index": (blob[:s["index_at"] + 3], "index at byte"),
        "behind_the_index": (blob[:s["footer_at"]], "stream footer at byte"),
        "inside_the_footer": (blob[:-3], "stream footer at byte"),
        "stream_header": (flipped(7, 0x01), "header CRC32 mismatch"),
        "block_header": (flipped(b0["at"] + 2), "block header CRC32 mismatch"),
        "index": (flipped(s["index_at"] + 2), "index CRC32 mismatch"),
        "footer": (flipped(s["footer_at"] + 5), "footer CRC32 mismatch"),
        "check": (flipped(b0["check_at"]), "check mismatch"),
        "lzma_data": (flipped(ch["at"] + ch["header"] + 40), "at byte"),
        "one_more_byte_of_text": (with_byte(ch["at"] + 2, (blob[ch["at"] + 2] + 1) & 0xff), "at byte"),
        "no_dictionary_reset": (with_byte(ch["at"], 0xC0 | (blob[ch["at"]] & 0x1f)), "a block's first chunk does not reset the dictionary"),
        "no_dictionary_reset_stored": (no_reset, "a block's first chunk does not reset the dictionary"),
        "lc_plus_lp_5": (with_byte(ch["at"] + 5, 4 + 9 * (1 + 5 * 2)), "bad LZMA properties (lc + lp > 4)"),
        "garbage_behind": (blob + b"garbage!", "bytes behind the last stream that are neither padding nor a stream"),
        "padding_of_six": (blob + bytes(6), "stream padding that is no multiple of four bytes"),
        "index_of_other_blocks": (blob[:s["index_at"]] + X.index_of([(a + 4, u) for a, u in s["records"]]) + blob[s["footer_at"]:],
                                  "index does not match the blocks"),
    }
    assert (blob[ch["at"] + 2] + 1) & 0xff   # (the size's low byte does not wrap)
    files = []
    for name, (data, word) in cases.items():
        files.append(str(tmp_path / f"{name}.xz"))
        open(files[-1], "wb").write(data)
    r = clean(subprocess.run([san] + files, capture_output=True, text=True))
    lines = r.stdout.split("\n")
    for (name, (_, word)), line in zip(cases.items(), lines):
        assert "\terror\t" in line and word in line, (name, line)


@pytest.mark.parametrize("kind,grouped", [("mt", True), ("reblocked", False), ("two_streams_padded", True)])
def test_two_thousand_damaged_copies_end_in_ok_or_an_error_line(san, texts, tmp_path, kind, grouped):
    """A bit flipped, the file cut short, a stretch copied elsewhere, 2 000 times with a fixed seed: every copy decodes or
    is refused in words (the program exits 3 on an error without words); a copy with a flipped bit that decodes holds the
    text; nothing is reported by the sanitizers."""
    p = str(tmp_path / "in.xz")
    open(p, "wb").write(inputs(texts, grouped)[kind][1])
    r = clean(subprocess.run([san, "--mutate", "11", "2000", p], capture_output=True, text=True))
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict((f.split("=")[0], int(f.split("=")[1])) for f in r.stdout.split())
    assert sum(got.values()) == 2_000 and got["flips_differ"] == 0 and got["errors"] > 1_000, got


def test_crc64_pieces_fold_to_the_serial_crc(san, texts, tmp_path):
    p = str(tmp_path / "text.bin")
    text = texts[(True, 1_000)]
    open(p, "wb").write(text)
    r = clean(subprocess.run([san, "--crc64", "5", "20", p], capture_output=True, text=True))
    lines = r.stdout.split()
    assert lines[:20] == ["ok"] * 20 and lines[20] == f"{X.crc64(text):016x}", lines
    assert X.crc64(b"123456789") == 0x995DC9BBDF1939FA   # (the check value of CRC-64/XZ)


def test_the_index_reader_returns_the_blocks(san, texts, tmp_path):
    for kind in ("mt", "two_streams_padded", "empty_stream", "one"):
        blob = inputs(texts, True)[kind][1]
        p = str(tmp_path / f"{kind}.xz")
        open(p, "wb").write(blob)
        r = clean(subprocess.run([san, "--index", p], capture_output=True, text=True))
        want = [(k, b["at"], b["unpadded"], b["text"]) for k, s in enumerate(X.walk(blob)) for b in s["blocks"]]
        assert [tuple(int(v) for v in ln.split("\t")) for ln in r.stdout.strip().split("\n") if ln] == want, kind
    for data in (blob[:-1], blob[:-12], blob[:-8] + bytes(8), b""):
        open(p, "wb").write(data)
        r = clean(subprocess.run([san, "--index", p], capture_output=True, text=True))
        assert r.returncode == 1 and r.stdout == "no index\n"
