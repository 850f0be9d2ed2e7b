"""The device decoders' kernels under AddressSanitizer and UBSan, on the CPU: tests/native/san_device_decoders.cpp linked with
the emulator's objects (the product's .hip sources, compiled by g++ with the sanitizers) into one stand-alone program,
built and run here; nothing is loaded into this process and no GPU is touched.  Per input form -- xz, zstd, gzip (a chunk
start every 2 048 bytes), bzip2, BGZF SAM, BGZF BAM, plain SAM text -- a good file of a small lifelike text
(tests/sam_lifelike.py) goes through the C ABI whole and in pieces of 1 .. 5 000 bytes, then TRIALS randomly damaged copies
of it: each ends in SLIMM_OK or an error in words, never in a sanitizer report.  The host decoders' own format code has its
programs already (san_xz, san_zstd, san_readers); this one covers the kernels around it (k_gz_*, k_zs_*, k_xz_decode,
k_bz2_*, the BGZF token kernels, k_sam_pieces / k_sam_decode, the BAM record finder), which otherwise run on the GPU only.

TRIALS = 100, the least the suite allows itself.  The times are indicative -- an 8-core machine, and other machines differ
several-fold --: the build (make -j8,
-O1 with both sanitizers) 65 s; the runs of 100 trials each: xz 1 s, zstd 5 s, gzip 50 s, bzip2 5 s, bgzf_sam 39 s, bgzf_bam
44 s, sam 1 s -- 145 s one after the other, 53 s side by side as the test runs them: about 120 s with the build.  For comparison,
there: tests/test_split_plan_sanitized.py 3 s and a fresh `make -C tests/native` 70 s, twice the two 146 s.

Found by it: k_inflate_decode (bgzf_tokens.hip) shifted by the extra-bit count of a "distance symbol" that behind a literal is
a literal's low byte (up to 126 bits: undefined, though the value was never used) -- on the GOOD BGZF files.  Its standing
case is test_good_bgzf_files_shift_by_less_than_a_word below."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import sam_lifelike as L
from tests.sam_lifelike import small_workload
from tests.sam_gz import bgzf, header_len

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
TRIALS, RECORDS = 100, 350
CODECS = ["xz", "zstd", "gzip", "bzip2", "bgzf_sam", "bgzf_bam", "sam"]


@pytest.fixture(scope="module")
def program():
    subprocess.run(["make", "-s", "-C", NATIVE, "-j", str(min(16, os.cpu_count() or 1)), "san_device_decoders"], check=True, capture_output=True)
    return os.path.join(NATIVE, "emu_build_san", "san_device_decoders")


def inputs(tmp_path):
    """{codec: (path, header bytes of the decoded form, records)}."""
    w = small_workload()
    text = L.lifelike_text(w, 5, hi_bytes=True)
    skip = header_len(text)
    bam, bam_skip, _ = L.lifelike_bam(w, 5, hi=20_000)
    ztext = L.zstd_text("l1")
    blobs = {
        "xz": (L.xz_copies(text)["preset6"], skip, RECORDS),
        "zstd": (L.zstd_golden("l1"), header_len(ztext), L.ZSTD_RECORDS),   # (its references are not the program's: records all the same)
        "gzip": (L.gzip_member(text, "mem1"), skip, RECORDS),
        "bzip2": (L.bzip2_copies(text)["two_streams"], skip, RECORDS),
        "bgzf_sam": (bgzf(text, seed=5, lo=500, hi=20_000), skip, RECORDS),
        "bgzf_bam": (bam, bam_skip, RECORDS),
        "sam": (text, skip, RECORDS),
    }
    out = {}
    for codec, (blob, sk, n) in blobs.items():
        p = str(tmp_path / f"good.{codec}")
        open(p, "wb").write(blob)
        out[codec] = (p, sk, n)
    return out


def run(program, files, codec, trials):
    path, skip, n = files[codec]
    env = dict(os.environ, SLIMM_FORCE="gzip_chunk=2048") if codec == "gzip" else {k: v for k, v in os.environ.items() if k != "SLIMM_FORCE"}
    return subprocess.run([program, codec, path, str(skip), str(n), str(trials), "11"], capture_output=True, text=True, timeout=600, env=env)


@pytest.mark.parametrize("codec", ["bgzf_sam", "bgzf_bam"])
def test_good_bgzf_files_shift_by_less_than_a_word(program, tmp_path, codec):
    """The case of the finding above: a lifelike BGZF file, undamaged.  Behind a literal k_inflate_decode reads a second symbol
    with the literal/length code, and computed a distance's extra bits from its low byte all the same: 66 .. 255 there gave a
    shift of 32 .. 126 bits, which UBSan reports.  Any text with letters shows it; write_sam's did too, but never ran here."""
    r = run(program, inputs(tmp_path), codec, 0)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip().endswith("total=0"), r.stdout


def test_damaged_files_end_in_words_never_in_a_sanitizer_report(program, tmp_path):
    files = inputs(tmp_path)

    with ThreadPoolExecutor(max_workers=min(len(CODECS), os.cpu_count() or 1)) as pool:
        results = dict(zip(CODECS, pool.map(lambda codec: run(program, files, codec, TRIALS), CODECS)))
    for codec, r in results.items():
        assert r.returncode == 0, (codec, r.returncode, r.stdout[-500:], r.stderr[-3000:])
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (codec, r.stderr[-3000:])
        assert r.stdout.strip().endswith(f"total={TRIALS}"), (codec, r.stdout)
