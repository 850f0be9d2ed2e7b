"""`slimm DB IN` on one synthetic name-grouped SAM file (slimm_amd/synth_bam.py: write_synthetic_sam) and its BGZF copy, read
by one context, by a group of two on one device through member 0 (`--devices 0,0`) and by the same group with every member
reading its own byte range (`--devices 0,0 --split-input`): seconds of every run, M records/s of the best, the
SLIMM_TRACE=cli lines of the split, and whether all the profiles agree.  --other DIR: the one-context runs also with the
`slimm` and `libslimm_hip.so` of another build (the commit before a change), interleaved with this build's.
python scripts/sam_split_cli.py [records] [processes for compressing] [--devices 0,0] [--runs 3] [--other DIR] [--json OUT]"""
import argparse, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.sam_gz_cli import bgzf_chunk, compress
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import _bgzf_block, write_sldb


def run(cli, args, out_stem, env_extra=None):
    env = dict(os.environ, SLIMM_TRACE="cli")
    env.pop("SLIMM_HIP_LIB", None)   # (every build finds its library next to its command)
    env.update(env_extra or {})
    t0 = time.time()
    r = subprocess.run([cli, "-w", "1000", "-o", out_stem] + args, capture_output=True, text=True, env=env)
    dt = time.time() - t0
    assert r.returncode == 0, r.stderr[-1500:]
    return dt, r.stderr


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("records", nargs="?", type=int, default=100_000_000)
    ap.add_argument("procs", nargs="?", type=int, default=16)
    ap.add_argument("--devices", default="0,0")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--other", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.records
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_split_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    info = write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    print(f"SAM: {n} records, {info['bytes'] / 1e9:.2f} GB of text, built in {info['seconds']:.0f} s", flush=True)
    files = {"plain SAM": sam, "BGZF SAM": sam + ".bgzf.gz"}
    t0 = time.time(); compress(sam, files["BGZF SAM"], bgzf_chunk, a.procs, _bgzf_block(b""))
    print(f"BGZF SAM: {os.path.getsize(files['BGZF SAM']) / 1e9:.2f} GB ({time.time() - t0:.0f} s)", flush=True)
    builds = {"this build": os.path.join(ROOT, "slimm_amd", "slimm")}
    if a.other:
        builds["other build"] = os.path.join(a.other, "slimm")
    modes = [("one context", [], list(builds)), (f"--devices {a.devices}", ["--devices", a.devices], ["this build"]),
             (f"--devices {a.devices} --split-input", ["--devices", a.devices, "--split-input"], ["this build"])]
    result, profiles, n_runs = {"records": n, "text_bytes": info["bytes"], "runs": {}}, set(), 0
    for label, path in files.items():
        for mode, extra, who in modes:
            times, last = {b: [] for b in who}, ""
            for k in range(a.runs):   # (the builds take turns, and turns at going first: what drifts over the visit drifts for both)
                for b in (who if k % 2 == 0 else who[::-1]):
                    n_runs += 1
                    d = os.path.join(tmp, f"out_{n_runs}") + "/"
                    os.makedirs(d, exist_ok=True)
                    dt, err = run(builds[b], extra + [db, path], d + "sample")
                    times[b].append(round(dt, 3))
                    profiles.add(open(d + "sample_profile.tsv").read())
                    last = err
            for b in who:
                best = min(times[b])
                print(f"   [{label}] {mode}, {b}: {' / '.join(f'{t:.3f}' for t in times[b])} s; best = {n / best / 1e6:.1f} M records/s "
                      f"({os.path.getsize(path) / best / 1e9:.2f} GB/s of the file)", flush=True)
                result["runs"][f"{label} | {mode} | {b}"] = times[b]
            if "--split-input" in extra:
                print("\n".join("      " + l[l.index("[trace]"):][:260] for l in last.splitlines() if "[trace] split" in l), flush=True)
    result["same_profile"] = len(profiles) == 1
    print("same profile:", result["same_profile"])
    if a.json:
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    for p in files.values():
        os.unlink(p)
