"""What the xz and zstd decoders say of damaged files, held word for word: tests/golden/codec_words holds, per codec, the error
of every one of 100 damaged copies of a committed input (tests/native/damaged_copies.h, seed 11) -- *_device.txt as the
device decoder's round refuses it (san_device_decoders with SAN_SHOW_WORDS, the kernels on the CPU), *_host.txt as the host
reader does (san_xz / san_zstd --words over the same copies).  The two paths name some places differently (a file cut inside
a chunk is the device's "block at byte 12: truncated" and the host's "chunk at byte N: truncated"): each keeps its words.
Recorded from the commit in front of the one that gave both paths one container walker each (zstd_walk.h, xz_walk.h).
Stand-alone programs under AddressSanitizer and UBSan; nothing is loaded into this process and no GPU is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
WORDS = os.path.join(ROOT, "tests", "golden", "codec_words")
TRIALS, SEED = 100, 11
# codec: (the input, header bytes of its decoded form, its records, the host program's sources)
INPUTS = {
    "xz": (os.path.join(ROOT, "tests", "golden", "xz", "long_grouped_one.sam.xz"), 476, 15_000, ("san_xz.cpp", "xz.cpp")),
    "zstd": (os.path.join(ROOT, "tests", "golden", "zstd_lifelike", "lifelike_grouped_l1.sam.zst"), 476, 300, ("san_zstd.cpp", "zstd.cpp")),
}


def recorded(name):
    return open(os.path.join(WORDS, name)).read().splitlines()


def clean(r):
    return r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


@pytest.mark.parametrize("codec", sorted(INPUTS))
def test_the_host_reader_keeps_its_words(tmp_path, codec):
    path, _, _, (program, reader) = INPUTS[codec]
    exe = str(tmp_path / program[:-4])
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(NATIVE, program), os.path.join(ROOT, "slimm_amd", "csrc", "host", reader), "-o", exe], check=True)
    r = subprocess.run([exe, "--words", str(SEED), str(TRIALS), path], capture_output=True, text=True, timeout=300)
    assert clean(r), r.stderr[-3000:]
    assert r.stdout.splitlines() == recorded(f"{codec}_host.txt")


@pytest.fixture(scope="module")
def device_program():
    subprocess.run(["make", "-s", "-C", NATIVE, "-j", str(min(16, os.cpu_count() or 1)), "san_device_decoders"], check=True, capture_output=True)
    return os.path.join(NATIVE, "emu_build_san", "san_device_decoders")


@pytest.mark.parametrize("codec", sorted(INPUTS))
def test_the_device_decoder_keeps_its_words(device_program, codec):
    path, skip, records, _ = INPUTS[codec]
    env = {k: v for k, v in os.environ.items() if k != "SLIMM_FORCE"}
    r = subprocess.run([device_program, codec, path, str(skip), str(records), str(TRIALS), str(SEED)], capture_output=True, text=True, timeout=600,
                       env=dict(env, SAN_SHOW_WORDS="1"))
    assert clean(r), r.stderr[-3000:]
    assert r.stdout.strip().endswith(f"total={TRIALS}"), r.stdout
    assert r.stderr.splitlines() == recorded(f"{codec}_device.txt")
