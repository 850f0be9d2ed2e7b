"""The sampled count's plain C++ (slimm_amd/csrc/tile_plan.h): the capacity rule cap(c) = S (c + k^2/2 + k sqrt(c + k^2/4)) + S,
the plan's choice of S, the bucket allocation and which slots of a range a sample takes, walked at their edges -- the sizes
at which S changes, capacities that just fit and just do not fit the allocation, c = 0, counts near 2^31, ranges of one
slot to thousands for every S -- with AddressSanitizer and UBSan: a stand-alone program,
tests/native/tile_sample_check.cpp, built and run here; nothing is loaded into this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capacities_strides_and_the_allocation(tmp_path):
    exe = str(tmp_path / "tile_sample_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "tile_sample_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("tile sample plan: ") and r.stdout.strip().endswith("checks ok"), r.stdout
