"""The lz4 code under AddressSanitizer and UBSan, on the CPU, as stand-alone programs (nothing is loaded into this process and
no GPU is touched): san_lz4 runs the host decoder and the container walker over good inputs, 100 damaged copies of each and
every truncation of their first 300 bytes; san_lz4_device (tests/native/san_lz4_device.cpp with the emulator's sanitized objects:
the product's .hip sources compiled by g++ against the host stand-in for the HIP runtime) pushes a good file whole and in pieces, then 100 damaged copies, through
slimm_push_lz4_sam_bytes -- k_lz4_tokens, k_lz4_expand, k_zs_double and k_zs_gather run on heap buffers of exact size.  Each
ends in SLIMM_OK or an error in words, never in a sanitizer report."""
import os
import subprocess

import pytest

from tests import sam_lifelike as LL
from tests import sam_lz4 as L
from tests.sam_gz import header_len
from tests.test_lz4_frame import made, san_lz4  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
TRIALS, RECORDS = 100, 350


def clean(r):
    return r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr


def test_host_decoder_and_walker_on_damaged_copies(san_lz4, tmp_path):  # noqa: F811
    m = made()
    blobs = {"linked9": L.golden("config1_grouped_linked9.sam.lz4"), "short": L.golden("short_grouped_b4.sam.lz4"),
             "lengths": m["inputs"]["lengths"][0], "frames": m["inputs"]["frames"][0], "linked_mixed": m["inputs"]["linked_mixed"][0]}
    for name, blob in blobs.items():
        p = str(tmp_path / f"{name}.lz4")
        open(p, "wb").write(blob)
        r = subprocess.run([san_lz4, "--damage", "11", str(TRIALS), p], capture_output=True, text=True, timeout=600)
        assert clean(r), (name, r.stderr[-3000:])
        assert r.stdout.strip().endswith("total=%d" % (TRIALS + min(300, len(blob)))), r.stdout


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The emulator's objects under the sanitizers (the Makefile's san_device_decoders target makes them all), linked with
    san_lz4_device.cpp."""
    import glob
    subprocess.run(["make", "-s", "-C", NATIVE, "-j", str(min(16, os.cpu_count() or 1)), "san_device_decoders"], check=True, capture_output=True)
    exe = str(tmp_path_factory.mktemp("san") / "san_lz4_device")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(NATIVE, "san_lz4_device.cpp")]
                   + sorted(glob.glob(os.path.join(NATIVE, "emu_build_san", "*.o"))), check=True)
    return exe


@pytest.mark.parametrize("kind", ["linked", "independent"])
def test_device_decoder_kernels_on_damaged_copies(program, tmp_path, kind):
    """A lifelike text of 350 records as a frame of the Python writer -- linked blocks with block checksums and a content
    checksum, or independent ones with nothing to check, so that damage reaches the kernels -- whole, in pieces of 1 .. 5 000
    bytes, and 100 damaged copies."""
    w = LL.small_workload()
    text = LL.lifelike_text(w, 5, hi_bytes=True)
    f = L.Frame(linked=kind == "linked").packed(text, step=20_000)
    blob = f.bytes(block_sums=kind == "linked", content_size=True, checksum=kind == "linked")
    p = str(tmp_path / "good.lz4")
    open(p, "wb").write(blob)
    env = {k: v for k, v in os.environ.items() if k != "SLIMM_FORCE"}
    r = subprocess.run([program, "lz4", p, str(header_len(text)), str(RECORDS), str(TRIALS), "11"], capture_output=True, text=True, timeout=600, env=env)
    assert clean(r), r.stderr[-3000:]
    assert r.stdout.strip().endswith("total=%d" % TRIALS), r.stdout
