"""The container walkers that the host readers and the device rounds share (slimm_amd/csrc/zstd_walk.h, xz_walk.h) under
AddressSanitizer and UBSan: a stand-alone program, tests/native/san_walkers.cpp, built and run here; nothing is loaded into
this process and no GPU is touched.  Over two committed inputs and 200 damaged copies of each, a walk gives the same items
and the same end whether the bytes come at once or in pieces (single bytes around every structural boundary, random pieces
of 1 .. 5 000 bytes, two halves); and a range that starts at any block of an xz file, told the stream's check kind, gets
back from the index exactly the records of the blocks in front of it.  About 3 s, the build included."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_a_walk_does_not_depend_on_where_the_bytes_are_cut(tmp_path):
    exe = str(tmp_path / "san_walkers")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    os.path.join(ROOT, "tests", "native", "san_walkers.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(GOLDEN, "xz", "long_grouped_one.sam.xz"), os.path.join(GOLDEN, "zstd_lifelike", "lifelike_grouped_l1.sam.zst"),
                        os.path.join(GOLDEN, "xz", "config1_grouped_mt.sam.xz")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = r.stdout.strip()
    assert out.startswith("xz: 201 files, ") and out.endswith(" range starts: ok"), out
    # (one block in the first xz file, more in the second: every one of them was a range's start)
    assert int(out.split(";")[-1].split()[0]) >= 3, out
