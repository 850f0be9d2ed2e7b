"""`slimm DB x.sam.xz` with xz SAM decoded on the device: the synthetic config-3 SAM text (slimm_amd/synth_bam.py) as
`xz -6 -T16 --block-size=8MiB` -- through the device decoder and, the baseline it has to beat, through `--host-decode` --
and as plain SAM and `zstd -3` for the distance: three runs each, alternated, every run under its own time limit, stopping at
the first failure.  With --rocprof DIR the xz kernels' times (`rocprofv3 --kernel-trace --stats`, in a run of its own).  The
machine's `xz` (and `zstd`) command is looked for, never fetched; without `xz` the script says so and stops.  The synthetic
text's compression ratio and block count describe that text only.
python scripts/sam_xz_cli.py [records] [--rocprof DIR] [--limit SECONDS] [--json FILE]"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
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
            if "k_xz_" in name:
                k = name[name.index("k_xz_"):].split("(")[0]
                calls, ns = out.get(k, (0, 0))
                out[k] = (calls + int(row["Calls"]), ns + int(float(row["TotalDurationNs"])))
    return out


def run(db, path, out, limit, extra=(), prefix=()):
    """One run of the command: (seconds, the trace lines); stops the script when it fails or takes longer than `limit`."""
    env = dict(os.environ, SLIMM_TRACE="cli")
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + list(prefix) + [CLI, "-w", "1000"] + list(extra) + ["-o", out, db, path], capture_output=True,
                       text=True, env=env)
    dt = time.time() - t0
    if r.returncode != 0:
        print(f"FAILED ({r.returncode}) on {path}:\n{r.stderr[-1500:]}", flush=True)
        sys.exit(1)
    return dt, [l[l.index("[trace]"):][:200] for l in r.stderr.splitlines() if "SAM on the device" in l or "read on the host" in l]


if __name__ == "__main__":
    args = sys.argv[1:]
    opts = {"--rocprof": None, "--limit": "600", "--json": None}
    for flag in opts:
        if flag in args:
            i = args.index(flag)
            opts[flag] = args[i + 1]
            del args[i:i + 2]
    prof, limit = opts["--rocprof"], int(opts["--limit"])
    n = int(args[0]) if args else 20_000_000
    tool = shutil.which("xz")
    if not tool:
        print("no `xz` command on this machine: nothing measured")
        sys.exit(2)
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_xz_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    t0 = time.time()
    xz_path = sam + ".xz"
    with open(xz_path, "wb") as f:
        jobs = [subprocess.Popen([tool, "-6", "-T16", "--block-size=8MiB", "-c", sam], stdout=f)]
    variants = [("plain SAM", sam, ()), ("xz device", xz_path, ()), ("xz --host-decode", xz_path, ("--host-decode",))]
    if shutil.which("zstd"):
        jobs.append(subprocess.Popen(["zstd", "-q", "-f", "-T8", "-3", sam, "-o", sam + ".zst"]))
        variants.append(("zstd -3", sam + ".zst", ()))
    else:
        print("no `zstd` command on this machine: that variant is left out")
    assert all(j.wait() == 0 for j in jobs)
    size = os.path.getsize(sam)
    print(f"{n} records: text {size / 1e9:.2f} GB -> xz {os.path.getsize(xz_path) / 1e9:.3f} GB (compressed in {time.time() - t0:.0f} s)", flush=True)
    times, profiles, traces = {k: [] for k, _, _ in variants}, set(), {}
    for k in range(3):
        for label, path, extra in variants:   # (alternated)
            out = os.path.join(tmp, f"run{k}_{label.replace(' ', '_')}_")
            dt, tr = run(db, path, out, limit, extra)
            times[label].append(dt)
            traces[label] = tr
            with open(glob.glob(out + "*profile.tsv")[0]) as f:
                profiles.add(f.read())
            print(f"   [{label}] {dt:.3f} s = {n / dt / 1e6:.2f} M records/s  {' | '.join(tr)}", flush=True)
    for label, ts in times.items():
        print(f"[{label}] {min(ts):.3f} - {max(ts):.3f} s", flush=True)
    print(f"one profile: {len(profiles) == 1}", flush=True)
    kernels = {}
    if prof:
        os.makedirs(prof, exist_ok=True)
        run(db, xz_path, os.path.join(tmp, "prof_"), limit, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "--"])
        for kname, (calls, ns) in sorted(kernel_stats(prof).items()):
            kernels[kname] = {"calls": calls, "ms": ns / 1e6}
            print(f"[xz] {kname}: {calls} calls, {ns / 1e6:.2f} ms = {size / max(ns, 1):.3f} GB/s of text", flush=True)
    if opts["--json"]:
        with open(opts["--json"], "w") as f:
            json.dump({"records": n, "text_bytes": size, "xz_bytes": os.path.getsize(xz_path), "seconds": times, "traces": traces,
                       "one_profile": len(profiles) == 1, "kernels": kernels}, f, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)
