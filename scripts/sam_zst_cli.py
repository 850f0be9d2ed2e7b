"""`slimm DB x.sam.zst` with zstd SAM decoded on the device: the synthetic config-3 SAM text (slimm_amd/synth_bam.py) as
`zstd -3` and `zstd -19`, and as plain SAM and default `gzip` for the distance -- three runs each, alternated, every run
under its own time limit, stopping at the first failure.  With --rocprof DIR the zstd kernels' times (`rocprofv3
--kernel-trace --stats`, in a run of its own).  The machine's `zstd` command is looked for, never fetched; without it the
script says so and stops.  The synthetic text's compression ratio describes that text only.
python scripts/sam_zst_cli.py [records] [--rocprof DIR] [--limit SECONDS]"""
import csv, glob, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import write_sldb

CLI = os.path.join(ROOT, "slimm_amd", "slimm")


def kernel_stats(d):
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = row.get("Name", "")
            if "k_zs_" in name:
                k = name[name.index("k_zs_"):].split("(")[0]
                calls, ns = out.get(k, (0, 0))
                out[k] = (calls + int(row["Calls"]), ns + int(float(row["TotalDurationNs"])))
    return out


def run(db, path, out, limit, prefix=()):
    """One run of the command: (seconds, the trace lines); stops the script when it fails or takes longer than `limit`."""
    env = dict(os.environ, SLIMM_TRACE="cli")
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [CLI, "-w", "1000", "-o", out, db, path], capture_output=True, text=True, env=env)
    dt = time.time() - t0
    if r.returncode != 0:
        print(f"FAILED ({r.returncode}) on {path}:\n{r.stderr[-1500:]}", flush=True)
        sys.exit(1)
    return dt, [l[l.index("[trace]"):][:200] for l in r.stderr.splitlines() if "SAM on the device" in l]


if __name__ == "__main__":
    args = sys.argv[1:]
    prof, limit = None, 300
    for flag in ("--rocprof", "--limit"):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            prof, limit = (v if flag == "--rocprof" else prof), (int(v) if flag == "--limit" else limit)
    n = int(args[0]) if args else 20_000_000
    tool = shutil.which("zstd")
    if not tool:
        print("no `zstd` command on this machine: nothing measured")
        sys.exit(2)
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_zst_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    t0 = time.time()
    files = {"plain SAM": sam, "zstd -3": sam + ".3.zst", "zstd -19": sam + ".19.zst", "gzip": sam + ".gz"}
    jobs = [subprocess.Popen([tool, "-q", "-f", "-T8", lvl, sam, "-o", out]) for lvl, out in (("-3", files["zstd -3"]), ("-19", files["zstd -19"]))]
    with open(files["gzip"], "wb") as g:
        jobs.append(subprocess.Popen(["gzip", "-c", sam], stdout=g))
    assert all(j.wait() == 0 for j in jobs)
    size = os.path.getsize(sam)
    print(f"{n} records: text {size / 1e9:.2f} GB -> " + ", ".join(f"{k} {os.path.getsize(p) / 1e9:.3f} GB" for k, p in files.items() if p != sam) +
          f" (compressed in {time.time() - t0:.0f} s)", flush=True)
    times, profiles = {k: [] for k in files}, set()
    for k in range(3):
        for label, path in files.items():   # (alternated)
            out = os.path.join(tmp, f"run{k}_{label.replace(' ', '_')}_")
            dt, tr = run(db, path, out, limit)
            times[label].append(dt)
            with open(glob.glob(out + "*profile.tsv")[0]) as f:
                profiles.add(f.read())
            print(f"   [{label}] {dt:.3f} s = {n / dt / 1e6:.2f} M records/s  {' | '.join(tr)}", flush=True)
    for label, ts in times.items():
        print(f"[{label}] {min(ts):.3f} - {max(ts):.3f} s", flush=True)
    print(f"one profile: {len(profiles) == 1}", flush=True)
    if prof:
        os.makedirs(prof, exist_ok=True)
        for label in ("zstd -3", "zstd -19"):
            d = os.path.join(prof, label.replace(" ", "").replace("-", "_l"))
            run(db, files[label], os.path.join(tmp, "prof_"), limit, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"])
            for kname, (calls, ns) in sorted(kernel_stats(d).items()):
                print(f"[{label}] {kname}: {calls} calls, {ns / 1e6:.2f} ms = {size / max(ns, 1):.2f} GB/s of text", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
