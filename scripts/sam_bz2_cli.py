"""`slimm DB IN` on one synthetic SAM file (slimm_amd/synth_bam.py: write_synthetic_sam) as plain SAM, BGZF SAM, bzip2 SAM
of many streams (one per 900 kB of text, as pbzip2 writes them) and -- for files of up to `single_max` records, as Python
compresses one stream on one core -- bzip2 SAM of one stream: M records/s, the command's push and decode times
(SLIMM_TRACE=cli), the device decoder's own split (SLIMM_TRACE=push), whether the profiles agree, and with --rocprof the
kernels' times from `rocprofv3 --kernel-trace --stats` in decoded GB/s.
The synthetic text repeats itself: it compresses far better than real reads do, and a block's time is not a real block's.
python scripts/sam_bz2_cli.py [records] [processes for compressing] [--single-max N] [--rocprof DIR]"""
import bz2, csv, glob, os, shutil, subprocess, sys, tempfile, time
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


def bz2_streams_chunk(args):   # one bzip2 stream per 900 kB of text (pbzip2's default)
    path, lo, hi = args
    with open(path, "rb") as f:
        f.seek(lo)
        data = f.read(hi - lo)
    return b"".join(bz2.compress(data[i:i + 900_000], 9) for i in range(0, len(data), 900_000))


def compress(path, out, fn, procs, tail=b""):
    size = os.path.getsize(path)
    with Pool(procs) as pool, open(out, "wb") as f:
        for blob in pool.imap(fn, [(path, lo, min(size, lo + CHUNK)) for lo in range(0, size, CHUNK)]):
            f.write(blob)
        f.write(tail)


def one_stream(path, out):
    c = bz2.BZ2Compressor(9)
    with open(path, "rb") as f, open(out, "wb") as g:
        while True:
            data = f.read(CHUNK)
            if not data:
                break
            g.write(c.compress(data))
        g.write(c.flush())


def kernel_stats(d):
    """{kernel: (calls, total ns)} of the bzip2 kernels from rocprofv3's kernel_stats.csv under d"""
    out = {}
    for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(p)):
            name = row.get("Name", "")
            if "k_bz2_" in name:
                k = name[name.index("k_bz2_"):].split("(")[0]
                calls, ns = out.get(k, (0, 0))
                out[k] = (calls + int(row["Calls"]), ns + int(float(row["TotalDurationNs"])))
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    single_max, prof = 5_000_000, None
    if "--single-max" in args:
        i = args.index("--single-max")
        single_max = int(args[i + 1])
        del args[i:i + 2]
    if "--rocprof" in args:
        i = args.index("--rocprof")
        prof = args[i + 1]
        del args[i:i + 2]
    n = int(args[0]) if args else 100_000_000
    procs = int(args[1]) if len(args) > 1 else 16
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_bz2_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    info = write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    files = {"plain SAM": sam, "BGZF SAM": sam + ".gz", "bzip2 SAM, streams": sam + ".streams.bz2"}
    t0 = time.time(); compress(sam, files["BGZF SAM"], bgzf_chunk, procs, _bgzf_block(b""))
    t1 = time.time(); compress(sam, files["bzip2 SAM, streams"], bz2_streams_chunk, procs)
    t2 = time.time()
    if n <= single_max:
        files["bzip2 SAM, one stream"] = sam + ".one.bz2"
        one_stream(sam, files["bzip2 SAM, one stream"])
    print(f"SAM: {n} records, {info['bytes'] / 1e9:.2f} GB of text; " +
          ", ".join(f"{k} {os.path.getsize(p) / 1e9:.3f} GB" for k, p in files.items()) +
          f" (compressed in {t1 - t0:.0f} / {t2 - t1:.0f} / {time.time() - t2:.0f} s)", flush=True)
    cli = os.path.join(ROOT, "slimm_amd", "slimm")
    outs = {}
    for label, path in files.items():
        d = os.path.join(tmp, label.replace(" ", "_").replace(",", "")) + "/"
        os.makedirs(d, exist_ok=True)
        best, tr = None, ""
        for _ in range(2):
            t0 = time.time()
            r = subprocess.run([cli, "-w", "1000", "-o", d + "sample", db, path], capture_output=True, text=True,
                               env=dict(os.environ, SLIMM_TRACE="cli,push" if "bzip2" in label else "cli"))
            dt_ = time.time() - t0
            assert r.returncode == 0, r.stderr[-1500:]
            if best is None or dt_ < best:
                best = dt_
                tr = "\n".join("      " + (l[l.index("[trace]"):] if "[trace]" in l else l)[:260] for l in r.stderr.splitlines()
                               if "[trace]" in l or "[push bzip2]" in l)
        outs[label] = open(d + "sample_profile.tsv").read()
        print(f"   slimm DB [{label}]: {best:.3f} s = {n / best / 1e6:.1f} M records/s ({os.path.getsize(path) / best / 1e9:.2f} GB/s of the file)\n{tr}",
              flush=True)
        if prof and "bzip2" in label:
            pd = os.path.join(prof, label.replace(" ", "_").replace(",", ""))
            shutil.rmtree(pd, ignore_errors=True)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", pd, "-o", "run", "--", cli, "-w", "1000", "-o",
                                d + "prof", db, path], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-1500:]
            for k, (calls, ns) in sorted(kernel_stats(pd).items()):
                print(f"      {k:14s} {calls:6d} calls {ns / 1e6:9.1f} ms = {info['bytes'] / ns:.2f} GB/s of decoded text", flush=True)
    print("same profile:", len(set(outs.values())) == 1)
    for label, p in files.items():
        os.unlink(p)
