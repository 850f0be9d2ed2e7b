"""`slimm DB x.sam.gz` with gzip SAM inflated on the device against a build that inflates it on the reader thread (the parent
commit's): the two builds alternated in one call, three runs each, every run under its own time limit, stopping at the
first failure.  Two files of the same records: the synthetic config-3 SAM text (slimm_amd/synth_bam.py) as default `gzip`,
and the same lines with read-like SEQ / QUAL (random bases, random qualities) that compress about 3-4-fold.  The synthetic
text compresses ~19-fold into few large blocks, so these numbers describe these two texts only.  Also: plain SAM and BGZF
SAM of the first text for the distance; with --rocprof DIR the gzip kernels' times (`rocprofv3 --kernel-trace --stats`, a
run of its own); with --sweep the chunk size (SLIMM_FORCE gzip_chunk) from 64 KiB to 1 MiB.
python scripts/sam_gz_device_cli.py --parent DIR [records] [--rocprof DIR] [--sweep] [--limit SECONDS]
DIR holds the other build's `slimm` and `libslimm_hip.so`."""
import csv, glob, os, random, shutil, subprocess, sys, tempfile, time, zlib
from multiprocessing import Pool
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import _bgzf_block, write_sldb

CHUNK = 64 << 20


def bgzf_chunk(args):
    path, lo, hi = args
    with open(path, "rb") as f:
        f.seek(lo)
        data = f.read(hi - lo)
    return b"".join(_bgzf_block(data[i:i + 65280]) for i in range(0, len(data), 65280))


def gzip_one_member(path, out):   # what `gzip x.sam` writes: level 6, one member, one core
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with open(path, "rb") as f, open(out, "wb") as g:
        while True:
            data = f.read(CHUNK)
            if not data:
                break
            g.write(c.compress(data))
        g.write(c.flush())


def read_like(path, out, seed=5):
    """The lines of `path` with SEQ and QUAL replaced by random bases and qualities of the same length."""
    rng = random.Random(seed)
    with open(path, "rb") as f, open(out, "wb") as g:
        for line in f:
            if line[:1] == b"@":
                g.write(line)
                continue
            fld = line.rstrip(b"\n").split(b"\t")
            n = len(fld[9]) if fld[9] != b"*" else 100
            fld[9] = bytes(rng.choices(b"ACGT", k=n))
            fld[10] = bytes(rng.choices(b"#,5:?FFFFFFF", k=n))
            g.write(b"\t".join(fld) + b"\n")


def kernel_stats(d):
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = row.get("Name", "")
            if "k_gz_" in name:
                k = name[name.index("k_gz_"):].split("(")[0]
                calls, ns = out.get(k, (0, 0))
                out[k] = (calls + int(row["Calls"]), ns + int(float(row["TotalDurationNs"])))
    return out


def run(build, db, path, out, limit, force=None):
    """One run of a build's command: (seconds, the trace lines); stops the script when it fails or takes longer than `limit`."""
    env = dict(os.environ, SLIMM_TRACE="cli")
    if build["lib"]:
        env["SLIMM_HIP_LIB"] = build["lib"]
    if force:
        env["SLIMM_FORCE"] = force
    t0 = time.time()
    r = subprocess.run(["timeout", "-k", "10", str(limit), build["cli"], "-w", "1000", "-o", out, db, path], capture_output=True, text=True, env=env)
    dt = time.time() - t0
    if r.returncode != 0:
        print(f"FAILED ({r.returncode}) {build['name']} on {path}:\n{r.stderr[-1500:]}", flush=True)
        sys.exit(1)
    return dt, [l[l.index("[trace]"):][:200] for l in r.stderr.splitlines() if "gzip SAM on the device" in l or "device decode" in l]


if __name__ == "__main__":
    args = sys.argv[1:]
    parent, prof, sweep, limit = None, None, False, 300
    for flag in ("--parent", "--rocprof", "--limit"):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            parent, prof, limit = (v if flag == "--parent" else parent), (v if flag == "--rocprof" else prof), (int(v) if flag == "--limit" else limit)
    if "--sweep" in args:
        sweep = True
        args.remove("--sweep")
    n = int(args[0]) if args else 20_000_000
    this = {"name": "this build", "cli": os.path.join(ROOT, "slimm_amd", "slimm"), "lib": None}
    builds = [this]
    if parent:
        builds = [{"name": "parent", "cli": os.path.join(parent, "slimm"), "lib": os.path.join(parent, "libslimm_hip.so")}, this]
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_gz_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    info = write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    reads = os.path.join(tmp, "reads.sam")
    read_like(sam, reads)
    t0 = time.time()
    with Pool(2) as pool:
        pool.starmap(gzip_one_member, [(sam, sam + ".gz"), (reads, reads + ".gz")])
    size = os.path.getsize(sam)
    with Pool(16) as pool, open(sam + ".bgzf.gz", "wb") as f:
        for blob in pool.imap(bgzf_chunk, [(sam, lo, min(size, lo + CHUNK)) for lo in range(0, size, CHUNK)]):
            f.write(blob)
        f.write(_bgzf_block(b""))
    print(f"{n} records: synthetic text {size / 1e9:.2f} GB -> gzip {os.path.getsize(sam + '.gz') / 1e9:.3f} GB; read-like text "
          f"{os.path.getsize(reads) / 1e9:.2f} GB -> gzip {os.path.getsize(reads + '.gz') / 1e9:.3f} GB (compressed in {time.time() - t0:.0f} s)", flush=True)
    profiles = {}
    for label, path, text in (("synthetic, gzip", sam + ".gz", sam), ("read-like, gzip", reads + ".gz", reads)):
        times = {b["name"]: [] for b in builds}
        for k in range(3):
            for b in builds:   # (alternated)
                out = os.path.join(tmp, f"{b['name'].replace(' ', '_')}_{k}_")
                dt, tr = run(b, db, path, out, limit)
                times[b["name"]].append(dt)
                profiles.setdefault(label, set()).add(open(out + "_profile.tsv").read() if os.path.exists(out + "_profile.tsv") else open(glob.glob(out + "*profile.tsv")[0]).read())
                print(f"   [{label}] {b['name']}: {dt:.3f} s = {n / dt / 1e6:.2f} M records/s  {' | '.join(tr)}", flush=True)
        for name, ts in times.items():
            print(f"[{label}] {name}: {min(ts):.3f} - {max(ts):.3f} s", flush=True)
        if parent:
            print(f"[{label}] every run of this build faster than every run of the parent: {max(times['this build']) < min(times['parent'])}", flush=True)
        print(f"[{label}] one profile: {len(profiles[label]) == 1}", flush=True)
    for label, path in (("synthetic, plain SAM", sam), ("synthetic, BGZF SAM", sam + ".bgzf.gz")):
        dt, _ = run(this, db, path, os.path.join(tmp, "other_"), limit)
        print(f"[{label}] this build: {dt:.3f} s = {n / dt / 1e6:.2f} M records/s", flush=True)
    if sweep:
        for kb in (64, 128, 256, 512, 1024):
            for label, path in (("synthetic", sam + ".gz"), ("read-like", reads + ".gz")):
                dt, tr = run(this, db, path, os.path.join(tmp, "sweep_"), limit, force=f"gzip_chunk={kb << 10}")
                print(f"[sweep] gzip_chunk = {kb} KiB, {label}: {dt:.3f} s  {' | '.join(tr)}", flush=True)
    if prof:
        for label, path, text in (("synthetic", sam + ".gz", sam), ("read-like", reads + ".gz", reads)):
            pd = os.path.join(prof, label)
            shutil.rmtree(pd, ignore_errors=True)
            r = subprocess.run(["timeout", "-k", "10", str(2 * limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", pd, "-o", "run", "--",
                                this["cli"], "-w", "1000", "-o", os.path.join(tmp, "prof_"), db, path], capture_output=True, text=True)
            if r.returncode != 0:
                print(f"FAILED rocprofv3 on {label}:\n{r.stderr[-1500:]}", flush=True)
                sys.exit(1)
            for k, (calls, ns) in sorted(kernel_stats(pd).items()):
                print(f"   [{label}] {k:14s} {calls:6d} calls {ns / 1e6:9.1f} ms = {os.path.getsize(text) / ns:.2f} GB/s of text", flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
