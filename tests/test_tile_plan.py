"""Which bucketing kernels a layout runs in each phase (slimm_amd/csrc/tile_plan.h), walked at the edges of its table and
under every SLIMM_FORCE key that moves a layout, with AddressSanitizer and UBSan: a stand-alone program,
tests/native/tile_plan_check.cpp, built and run here; nothing is loaded into this process.  That the library runs the
kernels of the path is held by the bracket counts of tests/test_gpu_layouts.py and by the parity tests that force each path."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_plan_at_the_edges_of_its_table(tmp_path):
    exe = str(tmp_path / "tile_plan_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "tile_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert r.stdout.startswith("tile plan: ") and r.stdout.strip().endswith("checks ok"), r.stdout
