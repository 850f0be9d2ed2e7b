"""`slimm -d` over a directory of BAMs: the files one after another (the command of the commit before --file-per-device, given
as --baseline) beside this tree's `--devices a,b,... --file-per-device`.
    python scripts/directory_cli.py --baseline PATH/slimm [--baseline-lib PATH/libslimm_hip.so] [--files 8] [--records 5000000]
                                    [--runs 3] [--easy] [--lists 0,0 0,0,0,0 ...]
The baseline is a build of the parent commit (git worktree add ../parent HEAD^ && make -C ../parent/slimm_amd/csrc); its
library is the one next to it unless --baseline-lib names one.
Builds the directory (config-3 records, one seed per file over one sample; slimm_amd/synth_bam.py, realistic unless --easy)
and reports the build time, which is outside the comparison.  One untimed reading of the directory warms the page cache;
then the variants alternate, --runs rounds of one run each, and every run's wall time -- process start to exit -- is printed,
with the median and the range of each variant at the end.  Every variant's output files are compared with the baseline's.
Default lists: 0,0 and 0,0,0,0, and 0,1,...,n-1 where the machine has n > 1 devices."""
import argparse, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_bam
from tests.bam_io import write_sldb

ap = argparse.ArgumentParser()
ap.add_argument("--baseline", required=True)
ap.add_argument("--baseline-lib")
ap.add_argument("--files", type=int, default=8)
ap.add_argument("--records", type=int, default=5_000_000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--easy", action="store_true")
ap.add_argument("--lists", nargs="*")
a = ap.parse_args()
if a.lists is None:
    a.lists = ["0,0", "0,0,0,0"]
    try:
        import torch
        if torch.cuda.device_count() > 1:
            a.lists.append(",".join(str(i) for i in range(torch.cuda.device_count())))
    except Exception:
        pass

tmp = tempfile.mkdtemp(prefix="slimm_dir_")
indir = os.path.join(tmp, "in")
os.makedirs(indir)
t0 = time.time()
size = 0
for k in range(a.files):
    w = make_workload(CONFIGS["config3"], seed=1 + k, sample_seed=1, n_records=a.records)
    if k == 0:
        write_sldb(os.path.join(tmp, "db.sldb"), w.taxonomy)
    info = write_synthetic_bam(os.path.join(indir, f"sample{k}.bam"), w.ref_names, w.ref_len, w.records, read_len=100, realistic=not a.easy)
    size += info["compressed_bytes"]
print(f"== {a.files} BAMs of {a.records} config-3 records ({'easy' if a.easy else 'realistic'}), {size / 1e9:.2f} GB in all, "
      f"built in {time.time() - t0:.0f} s (outside the comparison)", flush=True)

mine = os.path.join(ROOT, "slimm_amd", "slimm")
variants = [("parent -d --device 0", a.baseline, ["--device", "0"], dict(os.environ, SLIMM_HIP_LIB=a.baseline_lib) if a.baseline_lib else None)]
variants += [(f"--devices {l} --file-per-device", mine, ["--devices", l, "--file-per-device"], None) for l in a.lists]


def run(k):
    label, cli, extra, env = variants[k]
    out = os.path.join(tmp, f"out{k}") + "/"
    os.makedirs(out, exist_ok=True)
    t = time.perf_counter()
    r = subprocess.run([cli, "-d"] + extra + ["-w", "1000", "-o", out, os.path.join(tmp, "db.sldb"), indir], capture_output=True, text=True, env=env)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        sys.exit(f"{label}: FAILED\n{r.stderr[-2000:]}")
    return dt


run(0)   # (the warm-up reading: not in the figures)
times = [[] for _ in variants]
for rnd in range(a.runs):
    for k, v in enumerate(variants):
        times[k].append(run(k))
        print(f"   round {rnd + 1}: {v[0]}: {times[k][-1]:.3f} s", flush=True)
want = {f: open(os.path.join(tmp, "out0", f), "rb").read() for f in sorted(os.listdir(os.path.join(tmp, "out0")))}
for k, v in enumerate(variants):
    got = {f: open(os.path.join(tmp, f"out{k}", f), "rb").read() for f in sorted(os.listdir(os.path.join(tmp, f"out{k}")))}
    same = "the baseline's files, byte for byte" if got == want else "OUTPUTS DIFFER FROM THE BASELINE'S"
    t = times[k]
    print(f"== {v[0]}: median {statistics.median(t):.3f} s, range {min(t):.3f} - {max(t):.3f} s over {len(t)} runs = "
          f"{a.files * a.records / statistics.median(t) / 1e6:.1f} M records/s; {len(got)} output files: {same}", flush=True)
