"""The lzip code under AddressSanitizer and UBSan, on the CPU, as stand-alone programs (nothing is loaded into this process and
no GPU is touched): san_lzip runs the host decoder, the member finder -- whole and fed 1 000 bytes a peek -- and the backward
index over the committed files, the directed inputs, 200 damaged copies of each and every truncation of their first 300
bytes; san_lzip_device (tests/native/san_lzip_device.cpp with the emulator's sanitized objects: the product's .hip sources
compiled by g++ against the host stand-in for the HIP runtime) pushes a good file whole and in pieces, then 200 damaged copies,
through slimm_push_lzip_sam_bytes -- k_lzip_decode, k_xz_check and k_xz_fold run on heap buffers of exact size.  Each ends in
the exact text, SLIMM_OK or an error in words, never in a sanitizer report."""
import glob
import os
import subprocess

import pytest

from tests import sam_lifelike as LL
from tests import sam_lzip as Z
from tests.sam_gz import header_len
from tests.test_lzip_member import made, san_lzip  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
TRIALS, RECORDS = 200, 350


def clean(r):
    return r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr


def test_host_decoder_finder_and_index_on_damaged_copies(san_lzip, tmp_path):  # noqa: F811
    m = made()
    blobs = {"m17": Z.golden("config1_grouped_m17.sam.lz"), "d4k": Z.golden("short_grouped_d4k.sam.lz"), "empty_between": Z.golden("short_any_empty_between.sam.lz")}
    blobs.update({k: m["good"][k][0] for k in ("header_planted_in_the_payload", "length_273_ends_at_data_size", "distance_equal_to_the_dictionary")})
    for name, blob in blobs.items():
        p = str(tmp_path / f"{name}.lz")
        open(p, "wb").write(blob)
        r = subprocess.run([san_lzip, "--damage", "11", str(TRIALS), p], capture_output=True, text=True, timeout=600)
        assert clean(r), (name, r.stderr[-3000:])
        assert r.stdout.strip().endswith("total=%d" % (TRIALS + min(300, len(blob)))), r.stdout
    # every refused directed input and damage case: an error in words, no report
    bad = dict(m["bad"])
    bad.update({k: b for k, (b, _) in Z.damaged(m["texts"][(True, 1_000)])[1].items()})
    for name, blob in bad.items():
        p = str(tmp_path / "bad.lz")
        open(p, "wb").write(blob)
        r = subprocess.run([san_lzip, p], capture_output=True, text=True, timeout=60)
        assert clean(r) and "\terror\t" in r.stdout, (name, r.stdout, r.stderr[-3000:])


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The emulator's objects under the sanitizers (the Makefile's san_device_decoders target makes them all), linked with
    san_lzip_device.cpp."""
    subprocess.run(["make", "-s", "-C", NATIVE, "-j", str(min(16, os.cpu_count() or 1)), "san_device_decoders"], check=True, capture_output=True)
    exe = str(tmp_path_factory.mktemp("san") / "san_lzip_device")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(NATIVE, "san_lzip_device.cpp")]
                   + sorted(glob.glob(os.path.join(NATIVE, "emu_build_san", "*.o"))), check=True)
    return exe


@pytest.mark.parametrize("kind", ["members_of_20k", "d4k_with_an_empty_member"])
def test_device_decoder_kernels_on_damaged_copies(program, tmp_path, kind):
    """A lifelike text of 350 records in members of 20 000 bytes of text -- or with a 4 KiB dictionary, an empty member among
    them -- whole, in pieces of 1 .. 5 000 bytes, and 200 damaged copies."""
    w = LL.small_workload()
    text = LL.lifelike_text(w, 5, hi_bytes=True)
    blob = Z.members(text, 20_000) if kind == "members_of_20k" else Z.members(text[:30_000], 9_000, 4096) + Z.member(b"") + Z.members(text[30_000:], 50_000, 4096)
    assert Z.decode(blob) == text
    p = str(tmp_path / "good.lz")
    open(p, "wb").write(blob)
    env = {k: v for k, v in os.environ.items() if k != "SLIMM_FORCE"}
    r = subprocess.run([program, "lzip", p, str(header_len(text)), str(RECORDS), str(TRIALS), "11"], capture_output=True, text=True, timeout=900, env=env)
    assert clean(r), r.stderr[-3000:]
    assert r.stdout.strip().endswith("total=%d" % TRIALS), r.stdout
