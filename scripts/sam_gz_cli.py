"""`slimm DB IN` on one synthetic SAM file (slimm_amd/synth_bam.py: write_synthetic_sam) as plain SAM, BGZF SAM (`bgzip`: the
blocks cross the bus compressed and the device inflates them) and plain gzip SAM (one zlib stream on the reader thread):
M records/s and the SLIMM_TRACE=cli stage split of each, and whether the three profiles agree.
python scripts/sam_gz_cli.py [records] [processes for compressing]"""
import gzip, os, subprocess, sys, tempfile, time
from multiprocessing import Pool
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_sam
from tests.bam_io import _bgzf_block, write_sldb

CHUNK = 64 << 20


def bgzf_chunk(args):   # whole BGZF blocks of 65,280 bytes of text each (bgzip's block size)
    path, lo, hi = args
    with open(path, "rb") as f:
        f.seek(lo)
        data = f.read(hi - lo)
    return b"".join(_bgzf_block(data[i:i + 65280]) for i in range(0, len(data), 65280))


def gzip_chunk(args):   # one gzip member (a file of several members is one gzip file)
    path, lo, hi = args
    with open(path, "rb") as f:
        f.seek(lo)
        return gzip.compress(f.read(hi - lo), 6)


def compress(path, out, fn, procs, tail=b""):
    size = os.path.getsize(path)
    with Pool(procs) as pool, open(out, "wb") as f:
        for blob in pool.imap(fn, [(path, lo, min(size, lo + CHUNK)) for lo in range(0, size, CHUNK)]):
            f.write(blob)
        f.write(tail)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    procs = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
    tmp = tempfile.mkdtemp(prefix="slimm_sam_gz_")
    db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
    sam = os.path.join(tmp, "sample.sam")
    info = write_synthetic_sam(sam, w.ref_names, w.ref_len, w.records)
    del w
    files = {"plain SAM": sam, "BGZF SAM": sam + ".bgzf.gz", "gzip SAM": sam + ".gzip.gz"}
    t0 = time.time(); compress(sam, files["BGZF SAM"], bgzf_chunk, procs, _bgzf_block(b""))
    t1 = time.time(); compress(sam, files["gzip SAM"], gzip_chunk, procs)
    print(f"SAM: {n} records, {info['bytes'] / 1e9:.2f} GB of text, built in {info['seconds']:.0f} s; BGZF {os.path.getsize(files['BGZF SAM']) / 1e9:.2f} GB "
          f"({t1 - t0:.0f} s), gzip {os.path.getsize(files['gzip SAM']) / 1e9:.2f} GB ({time.time() - t1:.0f} s)", flush=True)
    cli = os.path.join(ROOT, "slimm_amd", "slimm")
    outs = {}
    for label, path in files.items():
        d = os.path.join(tmp, label.split()[0]) + "/"
        os.makedirs(d, exist_ok=True)
        best, tr = None, ""
        for _ in range(1 if label.startswith("gzip") else 2):
            t0 = time.time()
            r = subprocess.run([cli, "-w", "1000", "-o", d + "sample", db, path], capture_output=True, text=True,
                               env=dict(os.environ, SLIMM_TRACE="cli"))
            dt_ = time.time() - t0
            assert r.returncode == 0, r.stderr[-1500:]
            if best is None or dt_ < best:
                best, tr = dt_, "\n".join("      " + l[l.index("[trace]"):][:260] for l in r.stderr.splitlines() if "[trace]" in l)
        outs[label] = open(d + "sample_profile.tsv").read()
        print(f"   slimm DB [{label}]: {best:.3f} s = {n / best / 1e6:.1f} M records/s ({os.path.getsize(path) / best / 1e9:.2f} GB/s of the file)\n{tr}",
              flush=True)
    print("same profile:", len(set(outs.values())) == 1)
    for p in files.values():
        os.unlink(p)
