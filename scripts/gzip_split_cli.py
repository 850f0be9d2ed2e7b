"""`slimm DB IN.sam.gz` on a gzip copy (one member, zlib's default level, as `gzip x.sam` writes it) of the synthetic name-grouped
SAM file scripts/sam_cli.py uses (slimm_amd/synth_bam.py: write_synthetic_sam), read three ways: by one context (`--device 0`),
by four contexts on ONE device with every member reading its own bit range twice -- the window pass, then the text pass
(`--devices 0,0,0,0 --split-input`) --, and by four devices where four are there (`--devices 0,1,2,3 --split-input`).  Wall
seconds of every run, the spread, M records/s of the best, every member's share and the window pass's share (SLIMM_TRACE=cli),
and whether all the profiles agree.  --other DIR: the `slimm` and `libslimm_hip.so` of another build (the commit before this
change) read the file with `--devices 0,0,0,0 --split-input` as well -- its member-0 path --, the builds taking turns.  The
command's floor (slimm_gzip_split_floor, 32 MiB a member) is asked as ever unless --no-floor.  Every run is under its own
time limit; the script stops at the first failure.  The synthetic text repeats itself: its compression ratio, and so the
blocks per MB, describe this text only.
python scripts/gzip_split_cli.py [records] [--runs 3] [--members 4] [--other DIR] [--no-floor] [--limit SECONDS] [--json OUT]"""
import argparse, json, os, re, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import write_sldb

MEMBER = re.compile(r"split member (\d+): bytes \[(\d+), (\d+)\) of (\d+), (\d+) records, pread ([\d.]+) ms, push ([\d.]+) ms")
WINDOW_PASS = re.compile(r"gzip window pass: (\d+) members read their ranges in ([\d.]+) ms, the windows handed on in ([\d.]+) ms")


def gzip_copy(sam, out):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(sam, "rb") as f, open(out, "wb") as o:
        while True:
            piece = f.read(8 << 20)
            if not piece:
                break
            o.write(c.compress(piece))
        o.write(c.flush())


def devices_present():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 1


def run(cli, args, out_stem, limit, force):
    env = dict(os.environ, SLIMM_TRACE="cli")
    env.pop("SLIMM_HIP_LIB", None)   # (every build finds its library next to its command)
    env.pop("SLIMM_FORCE", None)
    if force:
        env["SLIMM_FORCE"] = force
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), cli, "-w", "1000", "-o", out_stem] + args, capture_output=True, text=True, env=env)
    dt = time.time() - t0
    if r.returncode != 0:
        print(f"FAILED ({r.returncode}): {' '.join(args)}\n{r.stderr[-1500:]}", flush=True)
        sys.exit(1)
    return dt, r.stderr


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("records", nargs="?", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--members", type=int, default=4)
    ap.add_argument("--other", default=None)
    ap.add_argument("--no-floor", action="store_true")
    ap.add_argument("--limit", type=int, default=180)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, G = a.records, a.members
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_gzip_split_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    info = write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    path = sam + ".gz"
    t0 = time.time(); gzip_copy(sam, path)
    os.unlink(sam)
    print(f"SAM: {n} records, {info['bytes'] / 1e9:.2f} GB of text; one gzip member at level 6: {os.path.getsize(path) / 1e6:.1f} MB "
          f"({time.time() - t0:.0f} s)", flush=True)
    force = "gzip_split_floor=0" if a.no_floor else None
    this, other = os.path.join(ROOT, "slimm_amd", "slimm"), (os.path.join(a.other, "slimm") if a.other else None)
    same = ",".join(["0"] * G)
    modes = [("--device 0", this, ["--device", "0"]), (f"--devices {same} --split-input", this, ["--devices", same, "--split-input"])]
    if other:
        modes.append((f"other build, --devices {same} --split-input (member 0 reads)", other, ["--devices", same, "--split-input"]))
    if devices_present() >= G:
        apart = ",".join(str(i) for i in range(G))
        modes.append((f"--devices {apart} --split-input", this, ["--devices", apart, "--split-input"]))
    else:
        print(f"   ({devices_present()} device(s) here: no run on {G} devices)", flush=True)
    result, profiles, times, best_err, n_runs = {"records": n, "text_bytes": info["bytes"], "file_bytes": os.path.getsize(path), "runs": {}, "members": {},
                                                "window_pass": {}, "cut": {}}, set(), {m[0]: [] for m in modes}, {}, 0
    for k in range(a.runs):   # (the modes take turns, and turns at going first: what drifts over the visit drifts for all)
        for mode, cli, extra in (modes if k % 2 == 0 else modes[::-1]):
            n_runs += 1
            d = os.path.join(tmp, f"out_{n_runs}") + "/"
            os.makedirs(d, exist_ok=True)
            dt, err = run(cli, extra + [db, path], d + "sample", a.limit, force)
            if not times[mode] or dt < min(times[mode]):
                best_err[mode] = err
            times[mode].append(round(dt, 3))
            profiles.add(open(d + "sample_profile.tsv").read())
    for mode, _, extra in modes:
        t, err = times[mode], best_err[mode]
        print(f"   {mode}: {' / '.join(f'{x:.3f}' for x in t)} s (spread {max(t) - min(t):.3f} s, median {sorted(t)[len(t) // 2]:.3f} s); "
              f"best = {n / min(t) / 1e6:.2f} M records/s", flush=True)
        result["runs"][mode] = t
        ms = [{"member": int(m[0]), "bytes": int(m[2]) - int(m[1]), "records": int(m[4]), "pread_ms": float(m[5]), "push_ms": float(m[6])} for m in MEMBER.findall(err)]
        result["members"][mode] = ms
        result["cut"][mode] = bool(ms) and "reading the file through member 0" not in err
        for m in ms:
            print(f"      member {m['member']}: {m['bytes'] / 1e6:8.1f} MB, {m['records']:10d} records, text pass: pread {m['pread_ms']:.0f} ms, push {m['push_ms']:.0f} ms", flush=True)
        wp = WINDOW_PASS.search(err)
        if wp:
            share = (float(wp.group(2)) + float(wp.group(3))) / 1e3 / min(t)
            result["window_pass"][mode] = {"members": int(wp.group(1)), "read_ms": float(wp.group(2)), "hand_on_ms": float(wp.group(3)), "share_of_best_run": round(share, 3)}
            print(f"      window pass: {wp.group(1)} members in {wp.group(2)} ms, handed on in {wp.group(3)} ms: {100 * share:.0f} % of the best run", flush=True)
        print("\n".join("      " + l[l.index("[trace]"):][:240] for l in err.splitlines() if "split input:" in l or "is not cut by byte range" in l), flush=True)
    result["same_profile"] = len(profiles) == 1
    print("same profile:", result["same_profile"])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
    os.unlink(path)
