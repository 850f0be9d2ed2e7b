#!/bin/bash
# AddressSanitizer + UBSan over the host code that does not need a GPU: the SAM/BAM/.sldb readers (good, truncated and
# corrupted inputs, 1 and 8 decode threads) and the host profile stages.  GPU sanitizers are not available on the pool,
# so this is the CPU-build sanitizer pass.  Usage: scripts/sanitize_host.sh [workdir]
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
W="${1:-/tmp/slimm_sanitize}"
mkdir -p "$W"
FLAGS="-std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer"
g++ $FLAGS "$ROOT/tests/native/san_readers.cpp" "$ROOT/slimm_amd/csrc/host/alignment_file.cpp" "$ROOT/slimm_amd/csrc/host/bzip2.cpp" \
    "$ROOT/slimm_amd/csrc/host/zstd.cpp" "$ROOT/slimm_amd/csrc/host/xz.cpp" "$ROOT/slimm_amd/csrc/host/sldb.cpp" -lz -lpthread -ldl -o "$W/san_readers"
g++ $FLAGS "$ROOT/tests/native/san_zstd.cpp" "$ROOT/slimm_amd/csrc/host/zstd.cpp" -o "$W/san_zstd"
g++ $FLAGS "$ROOT/tests/native/san_xz.cpp" "$ROOT/slimm_amd/csrc/host/xz.cpp" -o "$W/san_xz"
g++ $FLAGS -Wall -Wextra "$ROOT/tests/native/san_bgzf_block.cpp" -o "$W/san_bgzf_block"
g++ $FLAGS "$ROOT/tests/native/host_profile_bench.cpp" "$ROOT/slimm_amd/csrc/host_profile.cpp" -o "$W/san_profile"
g++ $FLAGS "$ROOT/slimm_amd/csrc/host/slimm_build_main.cpp" "$ROOT/slimm_amd/csrc/host/sldb.cpp" -lz -o "$W/san_build"
# ThreadSanitizer over the parallel BGZF inflate / record decode
g++ -std=c++17 -g -O1 -fsanitize=thread "$ROOT/tests/native/san_readers.cpp" "$ROOT/slimm_amd/csrc/host/alignment_file.cpp" \
    "$ROOT/slimm_amd/csrc/host/bzip2.cpp" "$ROOT/slimm_amd/csrc/host/zstd.cpp" "$ROOT/slimm_amd/csrc/host/xz.cpp" "$ROOT/slimm_amd/csrc/host/sldb.cpp" -lz -lpthread -ldl -o "$W/tsan_readers"
g++ -std=c++17 -g -O1 -fsanitize=thread -I"$ROOT/include" "$ROOT/slimm_amd/csrc/host/slimm_main.cpp" "$ROOT/slimm_amd/csrc/host/alignment_file.cpp" \
    "$ROOT/slimm_amd/csrc/host/bzip2.cpp" "$ROOT/slimm_amd/csrc/host/zstd.cpp" "$ROOT/slimm_amd/csrc/host/xz.cpp" "$ROOT/slimm_amd/csrc/host/sldb.cpp" -lz -lpthread -ldl -o "$W/tsan_slimm"
# the host emulator for a command whose threads drive several contexts at once (tests/native/emu_one_launch.cpp)
if [ -e "$ROOT/tests/native/libslimm_emu.so" ]; then
    g++ -std=c++17 -g -O1 -shared -fPIC -I"$ROOT/tests/native/hip_emu" "$ROOT/tests/native/emu_one_launch.cpp" -L"$ROOT/tests/native" \
        -Wl,--no-as-needed -lslimm_emu -Wl,-rpath,"$ROOT/tests/native" -ldl -o "$W/libslimm_emu_mt.so"
fi
cd "$ROOT"
python - "$W" <<'PY'
import os, subprocess, sys
sys.path.insert(0, os.getcwd())
from slimm_amd.synth import CONFIGS, make_workload
from tests.bam_io import write_bam, write_sam, write_sldb
from tests.cases import tiny_case, holes_case
d = sys.argv[1]
files = []
cases = [tiny_case(), holes_case(), make_workload(CONFIGS["config1"], seed=3),
         make_workload(CONFIGS["config2"], seed=4, n_records=150_000)]
for i, w in enumerate(cases):
    for fmt, wr in (("sam", write_sam), ("bam", write_bam)):
        p = f"{d}/c{i}.{fmt}"
        wr(p, w.ref_names, w.ref_len, w.records, read_len=w.avg_read_len)
        files.append(p)
    p = f"{d}/c{i}.sldb"
    write_sldb(p, w.taxonomy)
    files.append(p)
# (a BAM that hardly compresses: more than the reader's own first windows hold, so that read_raw reaches the part of the file it
# reads in place and read_blocks takes over)
write_bam(f"{d}/c4.bam", cases[3].ref_names, cases[3].ref_len, cases[3].records, read_len=cases[3].avg_read_len, irregular_seed=5)
files.append(f"{d}/c4.bam")
data = open(f"{d}/c2.bam", "rb").read()
open(f"{d}/trunc.bam", "wb").write(data[:len(data) // 3])
bad = bytearray(data); bad[200] ^= 0xff
open(f"{d}/flip.bam", "wb").write(bytes(bad))
open(f"{d}/short.sldb", "wb").write(open(f"{d}/c2.sldb", "rb").read()[:100])
open(f"{d}/garbage.sam", "w").write("@SQ\tSN:x\tLN:10\nr1\t0\tx\n")
files += [f"{d}/trunc.bam", f"{d}/flip.bam", f"{d}/short.sldb", f"{d}/garbage.sam"]
bad = 0
for thr in ("1", "8"):
    r = subprocess.run([f"{d}/san_readers"] + files, capture_output=True, text=True,
                       env=dict(os.environ, SAN_READER_THREADS=thr))
    print(r.stdout)
    if r.returncode or r.stderr.strip():
        bad += 1; print("SANITIZER OUTPUT:\n" + r.stderr)
r = subprocess.run([f"{d}/tsan_readers", f"{d}/c3.bam", f"{d}/c4.bam", f"{d}/c2.bam", f"{d}/trunc.bam"], capture_output=True, text=True,
                   env=dict(os.environ, SAN_READER_THREADS="8"))
print(r.stdout)
if r.returncode or r.stderr.strip():
    bad += 1; print("THREAD SANITIZER OUTPUT:\n" + r.stderr)
# the host zstd decoder: the committed inputs, written frames, and their truncated and bit-flipped copies
import random
from tests import sam_zst as Z
rng = random.Random(3)
zfiles = []
blobs = [Z.golden(n) for n in sorted(os.listdir(Z.GOLDEN)) if n.endswith(".zst")]
blobs += list(Z.written_copies(open(f"{d}/c2.sam", "rb").read()).values())
for k, blob in enumerate(blobs):
    copies = [blob] + [blob[:rng.randrange(1, len(blob))] for _ in range(20)]
    for _ in range(60):
        at = rng.randrange(len(blob))
        copies.append(blob[:at] + bytes([blob[at] ^ (1 << rng.randrange(8))]) + blob[at + 1:])
    for j, data in enumerate(copies):
        open(f"{d}/z{k}_{j}.zst", "wb").write(data)
        zfiles.append(f"{d}/z{k}_{j}.zst")
r = subprocess.run([f"{d}/san_zstd"] + zfiles, capture_output=True, text=True)
print(f"san_zstd: {len(zfiles)} files,", sum(1 for l in r.stdout.splitlines() if "\tok\t" in l), "decoded")
if r.returncode or r.stderr.strip():
    bad += 1; print("SANITIZER OUTPUT (san_zstd):\n" + r.stderr[-4000:])
# the host xz decoder (and the LZMA decoder the device runs): the committed inputs and written containers decoded, then
# damaged copies of three of them -- bits flipped, cut short, stretches copied elsewhere
from tests import sam_xz as X
short = X.case_text(d, True, 1_000)
xblobs = [X.golden(n) for n in sorted(os.listdir(X.GOLDEN)) if n.endswith(".xz")] + list(X.written_copies(short, "grouped").values())
xfiles = []
for k, blob in enumerate(xblobs):
    open(f"{d}/x{k}.xz", "wb").write(blob)
    xfiles.append(f"{d}/x{k}.xz")
r = subprocess.run([f"{d}/san_xz"] + xfiles, capture_output=True, text=True)
print(f"san_xz: {len(xfiles)} files,", sum(1 for l in r.stdout.splitlines() if "\tok\t" in l), "decoded")
if r.returncode or r.stderr.strip():
    bad += 1; print("SANITIZER OUTPUT (san_xz):\n" + r.stderr[-4000:])
for k in (0, len(xblobs) - 3, len(xblobs) - 2):
    r = subprocess.run([f"{d}/san_xz", "--mutate", "3", "3000", xfiles[k]], capture_output=True, text=True)
    print(f"san_xz --mutate {os.path.basename(xfiles[k])}:", r.stdout.strip())
    if r.returncode or r.stderr.strip():
        bad += 1; print("SANITIZER OUTPUT (san_xz --mutate):\n" + r.stderr[-4000:])
r = subprocess.run([f"{d}/san_bgzf_block"], capture_output=True, text=True)
print("san_bgzf_block:", r.stdout.strip().splitlines()[-1])
if r.returncode or r.stderr.strip():
    bad += 1; print("SANITIZER OUTPUT (san_bgzf_block):\n" + r.stdout + r.stderr[-4000:])
r = subprocess.run([f"{d}/san_profile"], capture_output=True, text=True)
print(r.stdout)
if r.returncode or r.stderr.strip():
    bad += 1; print("SANITIZER OUTPUT:\n" + r.stderr)
# slimm_build: well-formed dumps (plain and gzip'ed FASTA, tiny batches), then cut and garbled ones
import pathlib
from slimm_amd.synth import synth_taxonomy
from tests.ncbi_dumps import write_dumps
for k, (gz, batch) in enumerate([(False, "1000000"), (True, "7")]):
    t = pathlib.Path(d) / f"dumps{k}"
    t.mkdir(exist_ok=True)
    dd = write_dumps(t, synth_taxonomy(400, strain_level=bool(k), hole_every=3), gz_fasta=gz)
    runs = [dd]
    if k == 0:
        cut = dict(dd)
        for key in ("nodes", "names"):
            b = open(dd[key], "rb").read()
            open(dd[key] + ".cut", "wb").write(b[:len(b) // 2 + 3])
            cut[key] = dd[key] + ".cut"
        open(f"{t}/junk.a2t", "wb").write(b"\t\t\t\n\n\xff\xfe\t1\nACC000001\nACC000002\t\t99999999999999999999\n" + os.urandom(4096))
        cut["acc"] = [f"{t}/junk.a2t"] + dd["acc"]
        open(f"{t}/junk.fa", "wb").write(b">\n>>|\n@x\n" + os.urandom(2048) + b"\n>ACC000003.1 z")
        runs += [cut, dict(cut, fasta=f"{t}/junk.fa")]
    for rr in runs:
        r = subprocess.run([f"{d}/san_build", "-nm", rr["names"], "-nd", rr["nodes"], "-o", f"{t}/o.sldb", "-b", batch, rr["fasta"]]
                           + rr["acc"], capture_output=True, text=True, errors="replace")
        noise = [l for l in r.stderr.splitlines() if not l.startswith(("[MSG]", "[WARNING!]", "[VERBOSE"))]
        if r.returncode or noise:
            bad += 1; print("SANITIZER OUTPUT (slimm_build):\n" + r.stderr)
print("slimm_build under sanitizers: done")
# The `slimm` command itself under ThreadSanitizer -- its reader thread, the inflater and the pusher of the raw windows
# (RecordPump), the fallback to the host decoder -- with the HIP library replaced by the host emulator of tests/native (the
# command dlopen()s what SLIMM_HIP_LIB names).  Skipped when that library has not been built (make -C tests/native).
emu = os.path.join(os.getcwd(), "tests", "native", "libslimm_emu.so")
if os.path.exists(emu) and os.path.exists(f"{d}/tsan_slimm"):
    for extra in (["--window-mb", "1"], ["--window-mb", "3", "--no-mmap"], ["--host-decode"]):
        for inp in ("c3.bam", "c2.sam"):
            r = subprocess.run([f"{d}/tsan_slimm"] + extra + ["-w", "1000", "-o", f"{d}/cli_", f"{d}/{inp[:2]}.sldb", f"{d}/{inp}"], capture_output=True,
                               text=True, errors="replace", env=dict(os.environ, SLIMM_HIP_LIB=emu))
            if r.returncode or "ThreadSanitizer" in r.stderr:
                bad += 1; print("SANITIZER OUTPUT (slimm under TSan):\n" + r.stderr[-4000:])
    # --file-per-device: three slot threads over a directory of six files (the config-1 records in six parts, SAM and BAM),
    # each with its own reader, pump and context; the blocks of the log and the shared database are what they meet at.  The
    # emulator runs one kernel at a time: libslimm_emu_mt.so (built above) takes the launches of all threads in turn
    import numpy as np
    w = cases[2]
    os.makedirs(f"{d}/fpd_in", exist_ok=True)
    os.makedirs(f"{d}/fpd_out", exist_ok=True)
    cuts = [int(len(w.records) * c) for c in (0.0, 0.10, 0.25, 0.45, 0.60, 0.82, 1.0)]
    for k in range(6):
        (write_sam if k % 2 == 0 else write_bam)(f"{d}/fpd_in/s{k}.{'sam' if k % 2 == 0 else 'bam'}", w.ref_names, w.ref_len,
                                                 w.records.take(np.arange(cuts[k], cuts[k + 1])), read_len=w.avg_read_len)
    r = subprocess.run([f"{d}/tsan_slimm", "-d", "--devices", "0,0,0", "--file-per-device", "-ro", "-co", "-v", "-o", f"{d}/fpd_out/", f"{d}/c2.sldb",
                        f"{d}/fpd_in"], capture_output=True, text=True, errors="replace", env=dict(os.environ, SLIMM_HIP_LIB=f"{d}/libslimm_emu_mt.so", SLIMM_TRACE="cli"))
    if r.returncode or "ThreadSanitizer" in r.stderr or "5 handed to 3 slots" not in r.stderr:
        bad += 1; print("SANITIZER OUTPUT (slimm --file-per-device under TSan):\n" + r.stderr[-4000:])
    print("slimm (command, emulated device) under ThreadSanitizer: done")
print("sanitizer findings:", bad)
sys.exit(1 if bad else 0)
PY
