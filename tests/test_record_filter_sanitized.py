"""slimm_host_record_passes_bam / _sam (slimm_amd/csrc/record_filter.h) under AddressSanitizer and UBSan: a stand-alone
program, tests/native/san_record_filter.cpp, built and run here as a child process; nothing is loaded into this process and
nothing is preloaded.  Valid records and the same records damaged at random -- lengths overstated, tag types unknown, B counts
huge, records cut short -- each judged in an allocation of exactly its size.  What the verdicts must BE is held by
tests/test_record_filter_host.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sanitizer_program_ends_clean(tmp_path):
    exe = str(tmp_path / "san_record_filter")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_record_filter.cpp"), "-o", exe], check=True)
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert r.stdout.strip().endswith("damaged records judged: ok"), r.stdout
