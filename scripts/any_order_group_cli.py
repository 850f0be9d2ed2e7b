"""`slimm DB IN.bam` on the realistic synthetic BAM of scripts/realistic_cli.py in its UNSORTED copy (the reads interleaved at
random, @HD SO:unsorted): read by one context, by a group of two on one device (`--devices 0,0`: member 0's device decoders,
then the records dealt by key on the device) and by the same group with every member reading its own byte range (`--devices
0,0 --split-input`).  Seconds of every run, M records/s of the best, the SLIMM_TRACE=cli lines of the deal, whether all
profiles agree, and the partition kernels' own time on as many records (slimm_partition_by_key: kernel_ms).  --other DIR:
every mode also with the `slimm` and `libslimm_hip.so` of another build (the commit before a change), the two builds taking
turns.  Every run is a process of its own under a time limit; the first one that fails or runs out of time ends the script.
python scripts/any_order_group_cli.py [records] [--devices 0,0] [--runs 3] [--other DIR] [--json OUT] [--limit SECONDS]"""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_bam
from tests.bam_io import write_sldb


def run(cli, args, out_stem, limit):
    env = dict(os.environ, SLIMM_TRACE="cli")
    env.pop("SLIMM_HIP_LIB", None)   # (every build finds its library next to its command)
    t0 = time.time()
    r = subprocess.run([cli, "-w", "1000", "-o", out_stem] + args, capture_output=True, text=True, env=env, timeout=limit)
    dt = time.time() - t0
    if r.returncode != 0:   # (nothing more is started on the device after a run that failed)
        sys.exit(f"{cli} {' '.join(args)}: exit {r.returncode}\n{r.stderr[-1500:]}")
    return dt, r.stderr


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("records", nargs="?", type=int, default=100_000_000)
    ap.add_argument("--devices", default="0,0")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--other", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--limit", type=int, default=120)
    a = ap.parse_args()
    n = a.records
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_any_order_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    bam = os.path.join(tmp, "unsorted.bam")
    rec = w.records.take(np.random.default_rng(7).permutation(n))
    print(f"{n} records made and interleaved at random; writing the BAM", flush=True)
    info = write_synthetic_bam(bam, w.ref_names, w.ref_len, rec, read_len=100, hd="@HD\tVN:1.6\tSO:unsorted", realistic=True, threads=16)
    del w, rec
    print(f"unsorted BAM: {n} records, {info['raw_bytes'] / 1e9:.2f} GB of BAM in {info['compressed_bytes'] / 1e9:.2f} GB = "
          f"{info['raw_bytes'] / info['compressed_bytes']:.2f} x ({info['deflate']}), built in {info['seconds']:.0f} s", flush=True)
    builds = {"this build": os.path.join(ROOT, "slimm_amd", "slimm")}
    if a.other:
        builds["other build"] = os.path.join(a.other, "slimm")
    modes = [("one context", []), (f"--devices {a.devices}", ["--devices", a.devices]),
             (f"--devices {a.devices} --split-input", ["--devices", a.devices, "--split-input"])]
    result, profiles, n_runs = {"records": n, "file_bytes": info["compressed_bytes"], "runs": {}}, set(), 0
    for mode, extra in modes:
        who = list(builds)
        times, last = {b: [] for b in who}, ""
        for k in range(a.runs):   # (the builds take turns, and turns at going first: what drifts over the visit drifts for both)
            for b in (who if k % 2 == 0 else who[::-1]):
                n_runs += 1
                d = os.path.join(tmp, f"out_{n_runs}") + "/"
                os.makedirs(d, exist_ok=True)
                dt, err = run(builds[b], extra + [db, bam], d + "sample", a.limit)
                times[b].append(round(dt, 3))
                profiles.add(open(d + "sample_profile.tsv").read())
                if b == "this build":
                    last = err
        for b in who:
            best = min(times[b])
            print(f"   {mode}, {b}: {' / '.join(f'{t:.3f}' for t in times[b])} s; best = {n / best / 1e6:.1f} M records/s", flush=True)
            result["runs"][f"{mode} | {b}"] = times[b]
        print("\n".join("      " + l[l.index("[trace]"):][:260] for l in last.splitlines()
                        if "[trace] dealt by key" in l or "[trace] split member" in l or "[trace] device decode" in l), flush=True)
    result["same_profile"] = len(profiles) == 1
    print("same profile:", result["same_profile"])
    os.unlink(bam)
    # the partition kernels alone, on as many records with random keys: count 8 B read, scatter 22 B read + 22 B written a record
    from slimm_amd.profiler import partition_by_key
    rng = np.random.default_rng(1)
    key = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    ref = np.zeros(n, dtype=np.int32); pos = np.arange(n, dtype=np.int32); flag = np.zeros(n, dtype=np.uint16); chk = pos.view(np.uint32)
    result["partition_kernel_ms"] = {}
    for m in (2, 8):
        ms = [partition_by_key(key, ref, pos, flag, chk, m)[6] for _ in range(3)]
        print(f"   slimm_partition_by_key, {n} records, m = {m}: {' / '.join(f'{t:.3f}' for t in ms)} ms; best = "
              f"{52 * n / min(ms) / 1e9:.3f} TB/s on 52 B a record = {52 * n / min(ms) / 1e9 / 8:.3f} of 8 TB/s", flush=True)
        result["partition_kernel_ms"][str(m)] = [round(t, 4) for t in ms]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
