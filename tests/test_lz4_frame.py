"""CPU tests of the LZ4 format code (slimm_amd/csrc/lz4_frame.h, lz4_walk.h, host/lz4.cpp) through the stand-alone program
tests/native/san_lz4.cpp, built here under AddressSanitizer and UBSan: XXH32 against its known values (and the `xxhash`
module where the machine has it), the C++ container walker against the Python walker of tests/sam_lz4.py on every input,
the host decoder against the Python decoder and against what LZ4_decompress_safe gave when the fixtures were made
(tests/golden/lz4/directed_verdicts.json), and the committed fixtures against their texts.  No GPU is touched."""
import json
import os
import subprocess
import tempfile

import pytest

from tests import sam_lz4 as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.fixture(scope="module")
def san_lz4(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "san_lz4")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(NATIVE, "san_lz4.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", "lz4.cpp"), "-o", exe], check=True)
    return exe


_made = {}


def made():
    """The 50-record text's directed inputs, the 3 000- and 400-record texts and their fixtures: made once."""
    if not _made:
        with tempfile.TemporaryDirectory() as d:
            texts = {(g, n): L.case_text(d, g, n) for g, n in ((True, 50), (True, 3_000), (False, 3_000), (True, 400))}
        t = texts[(True, 50)]
        skip = L.header_len(t)
        _made.update(texts=texts, inputs=L.INPUTS(t[:skip], t[skip:]), invalid=L.INVALID(t[:skip], t[skip:]), header=t[:skip], records=t[skip:])
    return _made


def fixtures():
    m = made()
    out = {f"config1_{tag}_{key}.sam.lz4": m["texts"][(g, 3_000)] for g, tag in ((True, "grouped"), (False, "any")) for key in ("b4", "linked9", "default")}
    out["short_grouped_b4.sam.lz4"] = m["texts"][(True, 400)]
    return out


def run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    return r


def test_xxh32(san_lz4, tmp_path):
    """The empty input gives 0x02CC5D05; lengths 0 .. 40 and a long buffer, taken whole and in pieces, give the Python
    implementation's values, which are the `xxhash` module's where there is one."""
    try:
        import xxhash
    except ImportError:
        xxhash = None
    assert L.xxh32(b"") == 0x02CC5D05
    for n in list(range(41)) + [100_003]:
        data = bytes((i * 7 + 3) & 255 for i in range(n))
        if xxhash:
            assert L.xxh32(data) == xxhash.xxh32(data).intdigest(), n
        p = str(tmp_path / f"x{n}")
        open(p, "wb").write(data)
        for piece in (1 << 20, 1, 7, 16, 33):
            if n > 100 and piece == 1:
                continue
            assert run(san_lz4, "--xxh32", str(piece), p).stdout.strip() == "%08x" % L.xxh32(data), (n, piece)


def py_walk_lines(blob):
    out = []
    for f in L.walk(blob):
        if f["skippable"]:
            out.append(f"skippable {f['at']}")
            continue
        size = "-" if f["content_size"] is None else str(f["content_size"])
        out.append(f"frame {f['at']} {int(f['linked'])} {int(f['block_sums'])} {size} {f['block_max']}")
        out += [f"block {b['at']} {int(b['stored'])} {b['size']}" for b in f["blocks"]]
        out.append(f"end {f['end_at']}")
        if f["checksum_at"] is not None:
            out.append(f"sum {f['checksum_at']}")
    return out


def test_the_two_walkers_agree_and_the_host_decoder_gives_the_text(san_lz4, tmp_path):
    """Every directed input, every written copy and every committed fixture: lz4::Walker names the items the Python walker
    names, and the host decoder gives the text (the fixtures': the text made again from its seed)."""
    m = made()
    cases = {name: (blob, text) for name, (blob, text, _) in m["inputs"].items()}
    cases.update({name: (L.golden(name), text) for name, text in fixtures().items()})
    cases.update({"written_" + k: (b, m["texts"][(True, 400)]) for k, b in L.written_copies(m["texts"][(True, 400)]).items()})
    for name, (blob, text) in cases.items():
        p = str(tmp_path / "x.lz4")
        open(p, "wb").write(blob)
        assert run(san_lz4, "--walk", p).stdout.split("\n")[:-1] == py_walk_lines(blob), name
        assert L.decode(blob) == text, name
        r = run(san_lz4, p).stdout.split("\t")
        assert r[1:] == ["ok", str(len(text)), "%08x\n" % L.xxh32(text)], (name, r)


def test_the_fixtures_hold_what_they_are_named_for():
    """Stated by the walker, not by what the compressor was asked for."""
    for tag in ("grouped", "any"):
        b4, linked, default = (L.census(L.golden(f"config1_{tag}_{k}.sam.lz4")) for k in ("b4", "linked9", "default"))
        assert (b4["compressed"], b4["linked"], b4["block_sums"], b4["content_sums"]) == (7, 0, 0, 0) and b4["sequences"] > 9_000
        assert (linked["compressed"], linked["linked"], linked["block_sums"]) == (7, 1, 7) and linked["max_offset"] > 65_000
        assert L.walk(L.golden(f"config1_{tag}_linked9.sam.lz4"))[0]["content_size"] == 445_770 or tag == "any"
        assert (default["compressed"], default["content_sums"]) == (1, 1)
    short = L.census(L.golden("short_grouped_b4.sam.lz4"))
    assert short["compressed"] == 1 and short["stored"] == 0
    for name in os.listdir(L.GOLDEN):
        assert os.path.getsize(os.path.join(L.GOLDEN, name)) < 50_000, name


def test_invalid_inputs_are_refused_in_words_by_both(san_lz4, tmp_path):
    for name, (blob, words) in made()["invalid"].items():
        p = str(tmp_path / "x.lz4")
        open(p, "wb").write(blob)
        r = run(san_lz4, p).stdout.rstrip("\n").split("\t")
        assert r[1] == "error" and words in r[2] and r[2].startswith("block at byte "), (name, r)
        with pytest.raises(L.Bad):
            L.decode(blob)


def directed_blocks():
    import importlib.util
    spec = importlib.util.spec_from_file_location("lz4_make_inputs", os.path.join(L.GOLDEN, "make_inputs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    m = made()
    return mod.directed_blocks(m["header"], m["records"])


def test_blocks_against_the_recorded_verdicts_of_lz4_decompress_safe(san_lz4, tmp_path):
    """Every directed block: where LZ4_decompress_safe accepted it, the host decoder gives the recorded bytes; where it
    refused it and the host decoder takes it, the Python decoder gives the same text (the device: test_gpu_lz4_sam.py) --
    these are the blocks that break the format's end-of-block rules only.  A block of an invalid input is refused
    by all three."""
    verdicts = json.load(open(os.path.join(L.GOLDEN, "directed_verdicts.json")))
    blocks = directed_blocks()
    assert sorted(blocks) == sorted(verdicts)
    taken_though_refused = 0
    for name, body in blocks.items():
        v = verdicts[name]
        assert v["block"] == L.digest(body), name
        p = str(tmp_path / "b")
        open(p, "wb").write(body)
        r = run(san_lz4, "--block", str(1 << 16), p).stdout.rstrip("\n").split("\t")
        if name.startswith("invalid:") and "reaches_front" not in name and "beyond_first" not in name:
            assert r[0] == "error" and not v["accepted"], (name, r)
            continue
        if r[0] == "error":   # (a match in front of the block: alone, the block is refused by all)
            assert not v["accepted"] and ("reaches_front" in name or "beyond_first" in name), (name, r)
            continue
        text = bytes.fromhex(r[2]) if len(r) > 2 else b""
        if v["accepted"]:
            assert L.digest(text) == v["text"], name
        else:
            mine = bytearray()
            L.decode_block(body, mine, 0)
            assert bytes(mine) == text, name
            taken_though_refused += 1
        if L.LIB is not None:   # (where the machine has the library: the verdicts are still its)
            assert (L.decompress_safe(body, 1 << 17) is not None) == v["accepted"], name
    assert taken_though_refused >= 5
    assert all(not verdicts[f"taken:short_end_{k}"]["accepted"] for k in (3, 4, 5, 6, 7))
