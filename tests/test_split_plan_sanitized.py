"""What the four range planners of split.hip share (slimm_amd/csrc/split_plan.h) under AddressSanitizer and UBSan: a
stand-alone program, tests/native/san_split_plan.cpp, built and run here; nothing is loaded into this process.  The plans
themselves are held by tests/test_split_zstd_ranges.py and the ranges tests of tests/test_host_logic.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sanitizer_program_ends_clean(tmp_path):
    exe = str(tmp_path / "san_split_plan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_split_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip().endswith("4 paths: ok"), r.stdout
    assert sorted(os.listdir(tmp_path)) == ["san_split_plan"]   # (its file and its FIFO are gone)
