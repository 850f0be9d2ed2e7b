"""`slimm DB x.sam.lz4` with lz4 SAM decoded on the device: the synthetic config-3 SAM text (slimm_amd/synth_bam.py) as `lz4`
(independent 4 MiB blocks, a content checksum) and `lz4 -BD -9` (linked blocks), each read on the device and with
`--host-decode`, and as plain SAM for the distance -- three runs each, alternated, every run under its own time limit,
stopping at the first failure.  With --rocprof DIR the lz4 kernels' times (`rocprofv3 --kernel-trace --stats`, in a run of its
own).  The machine's `lz4` command is looked for, then its liblz4 (tests/sam_lz4.py's binding: frames of 64 MiB of text back
to back, with the command's settings), never fetched; without either the script says so and stops.  The synthetic text's
compression ratio describes that text only.
python scripts/sam_lz4_cli.py [records] [--rocprof DIR] [--limit SECONDS]"""
import csv, glob, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import write_sldb
from tests import sam_lz4 as L

CLI = os.path.join(ROOT, "slimm_amd", "slimm")
FRAME = 64 << 20
SETTINGS = {"lz4": dict(block_id=7, checksum=True), "lz4 -BD -9": dict(block_id=7, linked=True, level=9, checksum=True)}


def kernel_stats(d):
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = row.get("Name", "")
            for tag in ("k_lz4_", "k_zs_", "k_sam_"):
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
    return dt, [l[l.index("[trace]"):][:200] for l in r.stderr.splitlines() if "SAM on the device" in l]


def compress(tool, sam, label, out):
    if tool:
        subprocess.check_call([tool, "-q", "-f"] + label.split()[1:] + [sam, out])
        return
    with open(sam, "rb") as f, open(out, "wb") as g:
        while True:
            text = f.read(FRAME)
            if not text:
                break
            g.write(L.compress(text, **SETTINGS[label]))


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
    tool = shutil.which("lz4")
    if not tool and L.LIB is None:
        print("no `lz4` command and no liblz4 on this machine: nothing measured")
        sys.exit(2)
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_lz4_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    t0 = time.time()
    files = {"plain SAM": sam, "lz4": sam + ".lz4", "lz4 -BD -9": sam + ".9.lz4"}
    for label in SETTINGS:
        compress(tool, sam, label, files[label])
    size = os.path.getsize(sam)
    print(f"{n} records: text {size / 1e9:.2f} GB -> " + ", ".join(f"{k} {os.path.getsize(p) / 1e9:.3f} GB" for k, p in files.items() if p != sam) +
          f" (compressed by {'the lz4 command' if tool else 'liblz4, a frame per 64 MiB'} in {time.time() - t0:.0f} s)", flush=True)
    cases = [("plain SAM", ())] + [(label, extra) for label in SETTINGS for extra in ((), ("--host-decode",))]
    times, profiles = {}, set()
    for k in range(3):
        for label, extra in cases:   # (alternated)
            key = label + (" --host-decode" if extra else "")
            out = os.path.join(tmp, f"run{k}_{key.replace(' ', '_')}_")
            dt, tr = run(db, files[label], out, limit, extra)
            times.setdefault(key, []).append(dt)
            with open(glob.glob(out + "*profile.tsv")[0]) as f:
                profiles.add(f.read())
            print(f"   [{key}] {dt:.3f} s = {n / dt / 1e6:.2f} M records/s  {' | '.join(tr)}", flush=True)
    for key, ts in times.items():
        print(f"[{key}] {min(ts):.3f} - {max(ts):.3f} s", flush=True)
    print(f"one profile: {len(profiles) == 1}", flush=True)
    if prof:
        os.makedirs(prof, exist_ok=True)
        for label in SETTINGS:
            d = os.path.join(prof, label.replace(" ", "").replace("-", "_"))
            run(db, files[label], os.path.join(tmp, "prof_"), limit, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--"])
            for kname, (calls, ns) in sorted(kernel_stats(d).items()):
                print(f"[{label}] {kname}: {calls} calls, {ns / 1e6:.2f} ms = {size / max(ns, 1):.2f} GB/s of text", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
