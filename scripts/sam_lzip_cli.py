"""`slimm DB x.sam.lz` with lzip SAM decoded on the device: the synthetic config-3 SAM text (slimm_amd/synth_bam.py) as an lzip
file of members sized as `plzip`'s default (16 MiB of text each: twice its 8 MiB dictionary), read on the device and with
`--host-decode`, and as plain SAM for the distance -- three runs each, alternated, every run under its own time limit,
stopping at the first failure.  With --rocprof DIR the lzip kernels' times (`rocprofv3 --kernel-trace --stats`, in a run of its
own).  The members are written with Python's `lzma` (tests/sam_lzip.py: a raw LZMA1 stream ends in the marker lzip wants), a
process per core; no `lzip` or `plzip` command is needed, and none is fetched.  The synthetic text's compression ratio
describes that text only.
python scripts/sam_lzip_cli.py [records] [--rocprof DIR] [--limit SECONDS]"""
import csv, glob, os, shutil, subprocess, sys, tempfile, time
from concurrent.futures import ProcessPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import write_sldb
from tests import sam_lzip as Z

CLI = os.path.join(ROOT, "slimm_amd", "slimm")
DICT, MEMBER = 8 << 20, 16 << 20   # plzip's default dictionary, and the text it gives a member


def kernel_stats(d):
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = row.get("Name", "")
            for tag in ("k_lzip_", "k_xz_", "k_sam_"):
                if tag in name:
                    k = name[name.index(tag):].split("(")[0]
                    calls, ns = out.get(k, (0, 0))
                    out[k] = (calls + int(row["Calls"]), ns + int(float(row["TotalDurationNs"])))
    return out


def run(db, path, out, limit, extra=(), prefix=()):
    """One run of the command: (seconds, the trace lines); stops the script when it fails or takes longer than `limit`."""
    env = dict(os.environ, SLIMM_TRACE="cli")
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [CLI, "-w", "1000", "-o", out] + list(extra) + [db, path], capture_output=True, text=True, env=env)
    dt = time.time() - t0
    if r.returncode != 0 or "is not supported" in r.stderr:
        print(f"FAILED ({r.returncode}) on {path}:\n{r.stderr[-1500:]}", flush=True)
        sys.exit(1)
    return dt, [l[l.index("[trace]"):][:200] for l in r.stderr.splitlines() if "SAM on the device" in l or "read on the host" in l]


def member_at(args):
    sam, at = args
    with open(sam, "rb") as f:
        f.seek(at)
        return Z.member(f.read(MEMBER), DICT)


if __name__ == "__main__":
    args = sys.argv[1:]
    prof, limit = None, 300
    for flag in ("--rocprof", "--limit"):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            prof, limit = (v if flag == "--rocprof" else prof), (int(v) if flag == "--limit" else limit)
    n = int(args[0]) if args else 100_000_000
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_lzip_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    t0 = time.time()
    size = os.path.getsize(sam)
    lz = sam + ".lz"
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool, open(lz, "wb") as g:
        members = 0
        for blob in pool.map(member_at, [(sam, at) for at in range(0, size, MEMBER)]):
            g.write(blob)
            members += 1
    print(f"{n} records: text {size / 1e9:.2f} GB -> lzip {os.path.getsize(lz) / 1e9:.3f} GB in {members} members of {MEMBER >> 20} MiB of text "
          f"(written with Python's lzma in {time.time() - t0:.0f} s)", flush=True)
    cases = [("plain SAM", sam, ()), ("lzip", lz, ()), ("lzip --host-decode", lz, ("--host-decode",))]
    times, profiles = {}, set()
    for k in range(3):
        for key, path, extra in cases:   # (alternated)
            out = os.path.join(tmp, f"run{k}_{key.replace(' ', '_')}_")
            dt, tr = run(db, path, out, limit, extra)
            times.setdefault(key, []).append(dt)
            with open(glob.glob(out + "*profile.tsv")[0]) as f:
                profiles.add(f.read())
            print(f"   [{key}] {dt:.3f} s = {n / dt / 1e6:.2f} M records/s  {' | '.join(tr)}", flush=True)
    for key, ts in times.items():
        print(f"[{key}] {min(ts):.3f} - {max(ts):.3f} s", flush=True)
    print(f"one profile: {len(profiles) == 1}", flush=True)
    if prof:
        os.makedirs(prof, exist_ok=True)
        run(db, lz, os.path.join(tmp, "prof_"), limit, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "--"])
        for kname, (calls, ns) in sorted(kernel_stats(prof).items()):
            print(f"[lzip] {kname}: {calls} calls, {ns / 1e6:.2f} ms = {size / max(ns, 1):.2f} GB/s of text", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
