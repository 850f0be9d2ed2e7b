"""CPU tests of the layer that turns bits into bytes in the xz and zstd decoders, on inputs written on purpose
(tests/lzma_directed.py, tests/zstd_directed.py) and with a census that shows they reach what they claim (tests/lzma_paths.py,
tests/zstd_paths.py: decoders written from the formats' specifications that count the paths an input takes).  The census
decoders agree with lzma.decompress and libzstd on every committed input, and committed_inputs.json records what those inputs
reach.  Every directed input decodes to its text by the census decoder, by lzma / libzstd, by the host decoders (the stand-alone
sanitized programs san_xz and san_zstd) and by the device decoders' kernels on the CPU (san_device_decoders, under ASan and
UBSan); every input reaches the paths it is named for, and together they reach every path there is but the size-bounded ones
listed here.  Invalid variants are refused in words.  No GPU is touched."""
import json
import os
import subprocess

import pytest

from tests import codec_census, lzma_directed, lzma_paths, sam_xz as X, sam_zst as Z, zstd_directed, zstd_paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
RECORDS = 50

# What no valid stream of test size reaches -- size-bounded paths only -- and why.
XZ_BEYOND_TEST_SIZE = {f"slot:{k}": "a distance of more than 4 MiB: the inputs' largest dictionary, and text, is 4 MiB" for k in range(44, 64)}
ZSTD_BEYOND_TEST_SIZE = {
    **{f"of_code:{c}{e}": "an offset of 4 MiB or more: the inputs' largest window is 2 MiB, so that all inputs' text stays under 8 MiB"
       for c in range(22, 32) for e in ("", ":zeros", ":ones")},
    "of_code:21:ones": "an offset of 4 MiB - 4: beyond the 2 MiB window",
    "ll_code:35:ones": "131 071 literals and a match: more than the 128 KiB a block may regenerate",
    "ml_code:52:ones": "a match of 131 074 bytes: more than the 128 KiB a block may regenerate",
}


def _san(tmp_path_factory, name, source):
    exe = str(tmp_path_factory.mktemp("san") / name)
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(NATIVE, f"{name}.cpp"), os.path.join(ROOT, "slimm_amd", "csrc", "host", source), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def san_xz(tmp_path_factory):
    return _san(tmp_path_factory, "san_xz", "xz.cpp")


@pytest.fixture(scope="module")
def san_zstd(tmp_path_factory):
    return _san(tmp_path_factory, "san_zstd", "zstd.cpp")


@pytest.fixture(scope="module")
def device_program():
    subprocess.run(["make", "-s", "-C", NATIVE, "-j", str(min(16, os.cpu_count() or 1)), "san_device_decoders"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(NATIVE, "emu_build_san", "san_device_decoders")


_made = {}


def directed():
    """{"xz" / "zstd": (inputs, invalid variants)} over the 50-record text, made once; with its census per input."""
    if not _made:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            text = X.case_text(d, True, RECORDS)
        skip = X.header_len(text)
        for codec, mod, paths in (("xz", lzma_directed, lzma_paths), ("zstd", zstd_directed, zstd_paths)):
            ins = mod.INPUTS(text[:skip], text[skip:])
            for name, (blob, want, sk, _, _) in ins.items():
                assert want[sk:] == text[skip:] and want[:sk].endswith(b"\n"), (codec, name)
            _made[codec] = (ins, mod.INVALID(text[:skip], text[skip:]), {name: paths.decode(v[0]) for name, v in ins.items()})
    return _made


def clean(r):
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


# ---- the census decoders, and what the committed inputs reach
def test_the_census_decoders_agree_with_lzma_and_libzstd_on_every_committed_input():
    import lzma
    rows_xz, rows_zstd = codec_census.decoded("xz"), codec_census.decoded("zstd")
    assert len(rows_xz) == 24 + 5 and len(rows_zstd) == 14
    for name, blob, text, _ in rows_xz:
        assert text == lzma.decompress(blob), name
    if Z.LIB is not None:
        for name, blob, text, _ in rows_zstd:
            assert text == Z.decompress(blob, len(text) + 1), name
    # ... and committed_inputs.json is what they reach (python tests/golden/codec_paths/make_census.py writes it anew)
    assert json.load(open(codec_census.JSON)) == json.loads(json.dumps(codec_census.census(rows_xz, rows_zstd)))


def test_the_committed_inputs_leave_paths_unreached_that_the_directed_inputs_reach():
    """The reason for the directed inputs, kept true: should a committed input come to reach all of a codec's paths, this says so."""
    never = {k: set(v["never_reached"]) for k, v in json.load(open(codec_census.JSON)).items()}
    assert {"control:later:0xa0", "control:later:0xc0", "len:match:273", "len:rep:273", "slot:43", "reach:earlier_raw_chunk"} <= never["xz"]
    assert {"lit:rle:sf0:streams1", "huf:direct", "mode:ll:rle", "nseq:0", "nseq:3byte", "block:later:raw", "reps:carried_over_raw_block"} <= never["zstd"]


# ---- the directed inputs on the host
@pytest.mark.parametrize("codec", ["xz", "zstd"])
def test_every_directed_input_decodes_to_its_text_by_the_census_decoder_and_the_library(codec):
    ins, _, census = directed()[codec]
    for name, (blob, text, _, _, _) in ins.items():
        assert census[name][0] == text, name
        if codec == "xz":
            import lzma
            assert lzma.decompress(blob) == text, name
        elif Z.LIB is not None:
            assert Z.decompress(blob, len(text) + 1) == text, name


@pytest.mark.parametrize("codec", ["xz", "zstd"])
def test_every_directed_input_reaches_its_paths_and_together_they_reach_every_path(codec):
    ins, _, census = directed()[codec]
    mod, beyond = (lzma_paths, XZ_BEYOND_TEST_SIZE) if codec == "xz" else (zstd_paths, ZSTD_BEYOND_TEST_SIZE)
    known = set(mod.all_paths())
    total = set()
    for name, (_, _, _, paths, _) in ins.items():
        got = census[name][1]
        assert [p for p in paths if not got[p]] == [], name
        assert [p for p in paths if p not in known] == [], name
        total |= {p for p, n in got.items() if n}
    assert sorted(known - total) == sorted(beyond)
    assert all(reason for reason in beyond.values())
    # a check the decoder verifies on every input but the one made for the path without
    for name, (blob, _, _, _, _) in ins.items():
        if codec == "xz":
            checks = {s["check"] for s in X.walk(blob)}
            assert checks == {0} if name == "check_none" else checks <= {1, 4}, name
        else:
            assert all((f["checksum_at"] is None) == (name == "checksum_none") for f in Z.walk(blob)), name


def test_the_directed_inputs_stay_small():
    """A block of at most 64 KiB of text but for the far-distance inputs and the ones that must be larger by their subject (32 512
    sequences; the largest length codes); under 8 MiB of text for the inputs of both codecs together."""
    total = 0
    for codec, larger in (("xz", {"distance_slots"}), ("zstd", {"codes_and_extra_bits", "n_seq_32511", "n_seq_32512"})):
        ins = directed()[codec][0]
        total += sum(len(v[1]) for v in ins.values())
        for name, (blob, text, _, _, _) in ins.items():
            assert len(text) <= (1 << 16) or name in larger, (name, len(text))
    assert total < 8 << 20, total


@pytest.mark.parametrize("codec", ["xz", "zstd"])
def test_the_host_decoders_decode_every_directed_input_and_refuse_every_invalid_one_in_words(codec, san_xz, san_zstd, tmp_path):
    ins, invalid, _ = directed()[codec]
    san = san_xz if codec == "xz" else san_zstd
    out = str(tmp_path / "out.bin")
    for name, (blob, text, _, _, _) in ins.items():
        p = str(tmp_path / f"{name}.{codec}")
        open(p, "wb").write(blob)
        r = clean(subprocess.run([san, "--out", out, p], capture_output=True, text=True))
        assert r.returncode == 0, (name, r.stderr[-500:])
        assert open(out, "rb").read() == text, name
    files = []
    for name, (blob, _) in invalid.items():
        files.append(str(tmp_path / f"bad_{name}.{codec}"))
        open(files[-1], "wb").write(blob)
    r = clean(subprocess.run([san] + files, capture_output=True, text=True))
    lines = [ln for ln in r.stdout.split("\n") if ln]
    assert r.returncode == 0 and len(lines) == len(invalid), (r.returncode, r.stdout, r.stderr[-2000:])
    for (name, (_, words)), line in zip(invalid.items(), lines):
        assert "\terror\t" in line and words in line, (name, line)


@pytest.mark.parametrize("codec", ["xz", "zstd"])
def test_the_census_decoders_refuse_the_invalid_variants_too(codec):
    """... but for an LZMA chunk of control 0x80 behind an uncompressed one, which liblzma and the LZMA SDK decode: the
    encoders never write it, and this project asks for the state reset they write."""
    mod = lzma_paths if codec == "xz" else zstd_paths
    for name, (blob, _) in directed()[codec][1].items():
        if name == "control_0x80_behind_a_raw_chunk":
            continue
        with pytest.raises(mod.Bad):
            mod.decode(blob)


# ---- the device decoders' kernels on the CPU, under the sanitizers
def _device_run(program, codec, path, skip, records, force, leaks=True):
    env = {k: v for k, v in os.environ.items() if k != "SLIMM_FORCE"}
    if not leaks:   # (the program leaves at once, its context alive, when its good file is refused: that is no finding)
        env["ASAN_OPTIONS"] = "detect_leaks=0"
    if force:
        env["SLIMM_FORCE"] = force
    return subprocess.run([program, codec, path, str(skip), str(records), "0", "11"], capture_output=True, text=True, timeout=600, env=env)


@pytest.mark.parametrize("codec", ["xz", "zstd"])
def test_the_device_decoders_kernels_decode_every_directed_input_under_the_sanitizers(codec, device_program, tmp_path):
    """The good-file run of san_device_decoders (no damaged copies): whole and in pieces of 1 .. 5 000 bytes, RECORDS records;
    a history case once more under its force key, a round a block."""
    for name, (blob, _, skip, _, history) in directed()[codec][0].items():
        p = str(tmp_path / f"{name}.{codec}")
        open(p, "wb").write(blob)
        for force in [None] + ([history] if history else []):
            r = _device_run(device_program, codec, p, skip, RECORDS, force)
            assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (name, force, r.stderr[-3000:])
            assert r.stdout.strip().endswith("total=0"), (name, force, r.stdout)


@pytest.mark.parametrize("codec", ["xz", "zstd"])
def test_the_device_decoders_kernels_refuse_every_invalid_variant_in_words(codec, device_program, tmp_path):
    for name, (blob, words) in directed()[codec][1].items():
        p = str(tmp_path / f"bad_{name}.{codec}")
        open(p, "wb").write(blob)
        r = _device_run(device_program, codec, p, 0, RECORDS, None, leaks=False)
        assert r.returncode == 1 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (name, r.stderr[-3000:])
        assert "the good file in 1 pieces: rc -1" in r.stderr and words in r.stderr, (name, r.stderr[-500:])
