"""`slimm DB IN` on one synthetic name-grouped SAM file (slimm_amd/synth_bam.py: write_synthetic_sam) compressed as
`xz -6 -T16 --block-size=8MiB` (one stream, a block per 8 MiB of text), read by one context and by groups of 2, 4 and 8
contexts on ONE device with every member decoding the blocks of its own byte range (`--devices 0,0[,0...] --split-input`):
seconds of every run, the spread, M records/s of the best, every member's blocks and rounds (SLIMM_TRACE=push) and its share
(SLIMM_TRACE=cli), and whether all the profiles agree.  --other DIR: the one-context runs also with the `slimm` and
`libslimm_hip.so` of another build (the commit before this change), the two builds taking turns at going first, after one reading by each that is not
timed.  Every run is under its own time limit; the script stops at the first failure.  The file is written by the machine's `xz`; without one
the script says so and stops.  No speed-up is promised: one device's members share its CUs and its link.  The synthetic text
repeats itself: its compression ratio, and so a block's chunk and match counts, describe this text only.
python scripts/sam_xz_split_cli.py [records] [threads for compressing] [--members 2,4,8] [--runs 3] [--other DIR] [--limit SECONDS] [--json OUT]"""
import argparse, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import write_sldb

FILE = re.compile(r"\[push xz\] (\d+) streams, (\d+) blocks in (\d+) rounds;.*?; (\d+) compressed bytes -> (\d+) bytes of text; (\d+) index records checked")
STAMP = re.compile(r"\[push\s+([\d.]+)\] window (\d+): ([\d.]+) MB of text from xz")


def run(cli, args, out_stem, limit):
    env = dict(os.environ, SLIMM_TRACE="cli,push")
    env.pop("SLIMM_HIP_LIB", None)   # (every build finds its library next to its command)
    env.pop("SLIMM_FORCE", None)
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), cli, "-w", "1000", "-o", out_stem] + args, capture_output=True, text=True, env=env)
    dt = time.time() - t0
    if r.returncode != 0:
        print(f"FAILED ({r.returncode}): {' '.join(args)}\n{r.stderr[-1500:]}", flush=True)
        sys.exit(1)
    return dt, r.stderr


def members_of(err):
    """per context of the run, in the order they finished: streams, blocks, rounds, compressed and text bytes, index records"""
    return [{"streams": int(m[0]), "blocks": int(m[1]), "rounds": int(m[2]), "compressed_bytes": int(m[3]), "text_bytes": int(m[4]), "index_records": int(m[5])}
            for m in FILE.findall(err)]


def round_stamps(err):
    """when each window of xz text was handed over (ms since the process's first push line): rounds of several members
    that overlap in time show as interleaved stamps"""
    return [(float(t), int(w), float(mb)) for t, w, mb in STAMP.findall(err)]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("records", nargs="?", type=int, default=20_000_000)
    ap.add_argument("threads", nargs="?", type=int, default=16)
    ap.add_argument("--members", default="2,4,8")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--other", default=None)
    ap.add_argument("--limit", type=int, default=180)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if shutil.which("xz") is None:
        print("no xz on this machine: nothing measured")
        sys.exit(2)
    n = a.records
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_xz_split_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    info = write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    path = sam + ".xz"
    t0 = time.time()
    subprocess.run(["timeout", "-k", "10", "1200", "xz", "-6", f"-T{a.threads}", "--block-size=8MiB", sam], check=True)   # (replaces sample.sam)
    print(f"SAM: {n} records, {info['bytes'] / 1e9:.2f} GB of text; xz -6 -T{a.threads} --block-size=8MiB: {-(-info['bytes'] // (8 << 20))} blocks, "
          f"{os.path.getsize(path) / 1e9:.3f} GB ({time.time() - t0:.0f} s)", flush=True)
    builds = {"this build": os.path.join(ROOT, "slimm_amd", "slimm")}
    if a.other:
        builds["other build"] = os.path.join(a.other, "slimm")
    for b, cli in builds.items():   # (one reading each that is not timed: no build pays for the page cache or the device's first use)
        os.makedirs(os.path.join(tmp, "warm"), exist_ok=True)
        run(cli, [db, path], os.path.join(tmp, "warm", "sample"), a.limit)
    modes = [("one context", [], list(builds))]
    for g in (int(x) for x in a.members.split(",") if x):
        devs = ",".join(["0"] * g)
        modes.append((f"{g} contexts, --split-input", ["--devices", devs, "--split-input"], ["this build"]))
    result, profiles, n_runs = {"records": n, "text_bytes": info["bytes"], "file_bytes": os.path.getsize(path), "runs": {}, "members": {}, "windows": {}}, set(), 0
    for mode, extra, who in modes:
        times, best_err = {b: [] for b in who}, {}
        for k in range(a.runs):   # (the builds take turns, and turns at going first: what drifts over the visit drifts for both)
            for b in (who if k % 2 == 0 else who[::-1]):
                n_runs += 1
                d = os.path.join(tmp, f"out_{n_runs}") + "/"
                os.makedirs(d, exist_ok=True)
                dt, err = run(builds[b], extra + [db, path], d + "sample", a.limit)
                if not times[b] or dt < min(times[b]):
                    best_err[b] = err
                times[b].append(round(dt, 3))
                profiles.add(open(d + "sample_profile.tsv").read())
        for b in who:
            t = times[b]
            print(f"   {mode}, {b}: {' / '.join(f'{x:.3f}' for x in t)} s (spread {max(t) - min(t):.3f} s, median {sorted(t)[len(t) // 2]:.3f} s); "
                  f"best = {n / min(t) / 1e6:.2f} M records/s", flush=True)
            result["runs"][f"{mode} | {b}"] = t
            ms = members_of(best_err[b])
            result["members"][f"{mode} | {b}"] = ms
            stamps = round_stamps(best_err[b])
            result["windows"][f"{mode} | {b}"] = stamps
            for m in ms:
                print(f"      {m['blocks']:5d} blocks of {m['streams']} streams in {m['rounds']:3d} rounds: {m['compressed_bytes'] / 1e6:9.1f} MB -> "
                      f"{m['text_bytes'] / 1e6:9.1f} MB of text, {m['index_records']} index records checked", flush=True)
            if stamps:
                print("      windows handed over at (ms): " + " ".join(f"{t:.0f}" for t, _, _ in stamps[:64]), flush=True)
            if extra:
                err = best_err[b]
                print("\n".join("      " + l[l.index("[trace]"):][:240] for l in err.splitlines()
                                if "[trace] split member" in l or "split input:" in l or "is not cut by byte range" in l), flush=True)
                result.setdefault("fell_back", {})[mode] = "device decode on member 0" in err
    result["same_profile"] = len(profiles) == 1
    print("same profile:", result["same_profile"])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    os.unlink(path)
