"""`slimm DB IN` on one synthetic name-grouped SAM file (slimm_amd/synth_bam.py: write_synthetic_sam) compressed as bzip2
streams of 900 kB of text each (as pbzip2 writes them), read by one context and by groups of 2, 4 and 8 contexts on ONE device
with every member decoding the blocks of its own byte range (`--devices 0,0[,0...] --split-input`): seconds of every run, the
spread, M records/s of the best, every member's decode / inverse BWT / emit times (SLIMM_TRACE=push) and its share
(SLIMM_TRACE=cli), and whether all the profiles agree.  --other DIR: the one-context runs also with the `slimm` and
`libslimm_hip.so` of another build (the commit before this change), the two builds taking turns at going first.
The synthetic text repeats itself: it compresses far better than real reads do, and a block's time is not a real block's.
python scripts/sam_bz2_split_cli.py [records] [processes for compressing] [--members 2,4,8] [--runs 3] [--other DIR] [--json OUT]"""
import argparse, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.sam_bz2_cli import bz2_streams_chunk, compress
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import write_sldb

PUSH = re.compile(r"\[push bzip2\] (\d+) streams, (\d+) blocks in (\d+) batches, (\d+) false magics; find ([\d.]+) ms, decode ([\d.]+) ms, "
                  r"inverse BWT ([\d.]+) ms, text ([\d.]+) ms")


def run(cli, args, out_stem):
    env = dict(os.environ, SLIMM_TRACE="cli,push")
    env.pop("SLIMM_HIP_LIB", None)   # (every build finds its library next to its command)
    t0 = time.time()
    r = subprocess.run([cli, "-w", "1000", "-o", out_stem] + args, capture_output=True, text=True, env=env)
    dt = time.time() - t0
    assert r.returncode == 0, r.stderr[-1500:]
    return dt, r.stderr


def members_of(err):
    """per context of the run, in the order they finished: blocks, batches, and the milliseconds of the three stages"""
    return [{"blocks": int(m[1]), "batches": int(m[2]), "decode_ms": float(m[5]), "inverse_bwt_ms": float(m[6]), "emit_ms": float(m[7])}
            for m in PUSH.findall(err)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("records", nargs="?", type=int, default=5_000_000)
    ap.add_argument("procs", nargs="?", type=int, default=16)
    ap.add_argument("--members", default="2,4,8")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--other", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.records
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_bz2_split_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    info = write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    path = sam + ".streams.bz2"
    t0 = time.time(); compress(sam, path, bz2_streams_chunk, a.procs)
    os.unlink(sam)
    print(f"SAM: {n} records, {info['bytes'] / 1e9:.2f} GB of text; bzip2 streams: {os.path.getsize(path) / 1e9:.3f} GB ({time.time() - t0:.0f} s)", flush=True)
    builds = {"this build": os.path.join(ROOT, "slimm_amd", "slimm")}
    if a.other:
        builds["other build"] = os.path.join(a.other, "slimm")
    modes = [("one context", [], list(builds))]
    for g in (int(x) for x in a.members.split(",") if x):
        devs = ",".join(["0"] * g)
        modes.append((f"{g} contexts, --split-input", ["--devices", devs, "--split-input"], ["this build"]))
    result, profiles, n_runs = {"records": n, "text_bytes": info["bytes"], "file_bytes": os.path.getsize(path), "runs": {}, "members": {}}, set(), 0
    for mode, extra, who in modes:
        times, best_err = {b: [] for b in who}, {}
        for k in range(a.runs):   # (the builds take turns, and turns at going first: what drifts over the visit drifts for both)
            for b in (who if k % 2 == 0 else who[::-1]):
                n_runs += 1
                d = os.path.join(tmp, f"out_{n_runs}") + "/"
                os.makedirs(d, exist_ok=True)
                dt, err = run(builds[b], extra + [db, path], d + "sample")
                if not times[b] or dt < min(times[b]):
                    best_err[b] = err
                times[b].append(round(dt, 3))
                profiles.add(open(d + "sample_profile.tsv").read())
        for b in who:
            t = times[b]
            print(f"   {mode}, {b}: {' / '.join(f'{x:.3f}' for x in t)} s (spread {max(t) - min(t):.3f} s); best = {n / min(t) / 1e6:.2f} M records/s",
                  flush=True)
            result["runs"][f"{mode} | {b}"] = t
            ms = members_of(best_err[b])
            result["members"][f"{mode} | {b}"] = ms
            for m in ms:
                print(f"      {m['blocks']:5d} blocks in {m['batches']:3d} batches: decode {m['decode_ms']:8.1f} ms, inverse BWT {m['inverse_bwt_ms']:8.1f} ms, "
                      f"emit {m['emit_ms']:8.1f} ms", flush=True)
            if extra:
                err = best_err[b]
                print("\n".join("      " + l[l.index("[trace]"):][:240] for l in err.splitlines() if "[trace] split member" in l or "split input:" in l), flush=True)
                result.setdefault("fell_back", {})[mode] = "device decode on member 0" in err
    result["same_profile"] = len(profiles) == 1
    print("same profile:", result["same_profile"])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    os.unlink(path)
