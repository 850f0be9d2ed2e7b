"""What the record filter costs in the `slimm` command, on the BAM that compresses like a BAM (slimm_amd/synth_bam.py,
realistic=True; scripts/realistic_cli.py's file) with an MD and an NM tag behind every record:
    python scripts/record_filter_cli.py [records] [runs]
`slimm DB IN.bam`, process start to profile written, `runs` times each (default 3), the variants taken in turn:
    no option;  -q 10 --exclude-flags 0xF00;  --min-aligned 50 --min-identity 0.95
and, when SLIMM_OTHER_CLI names another build's `slimm` (the parent commit's, beside its own libslimm_hip.so), that one
without options too.  Every record has MAPQ 255, CIGAR 100M and NM 2: the second filter walks every record's CIGAR and tags and
drops none, so the work behind the decoders is the same in the three.  Prints every wall time and the stage trace of each
variant's best run."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slimm_amd.synth import CONFIGS, make_workload
from slimm_amd.synth_bam import write_synthetic_bam
from tests.bam_io import write_sldb

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
w = make_workload(CONFIGS["config3"], seed=1, n_records=n)
tmp = tempfile.mkdtemp(prefix="slimm_rf_")
db = os.path.join(tmp, "db.sldb"); write_sldb(db, w.taxonomy)
bam = os.path.join(tmp, "realistic.bam")
info = write_synthetic_bam(bam, w.ref_names, w.ref_len, w.records, read_len=100, realistic=True, tags=b"MDZ48A51\0NMC\x02")
print(f"== {n} records, {info['raw_bytes'] / 1e9:.2f} GB of BAM in {info['compressed_bytes'] / 1e9:.2f} GB = "
      f"{info['raw_bytes'] / info['compressed_bytes']:.2f} x ({info['deflate']}), built in {info['seconds']:.0f} s", flush=True)
cli = os.path.join(ROOT, "slimm_amd", "slimm")
variants = [("no option", cli, []), ("-q 10 --exclude-flags 0xF00", cli, ["-q", "10", "--exclude-flags", "0xF00"]),
            ("--min-aligned 50 --min-identity 0.95", cli, ["--min-aligned", "50", "--min-identity", "0.95"])]
if os.environ.get("SLIMM_OTHER_CLI"):
    variants.insert(0, ("other build, no option", os.environ["SLIMM_OTHER_CLI"], []))
times = {v[0]: [] for v in variants}
best = {}
profiles = {}
for r in range(runs + 1):   # (the first round warms the page cache and is not counted)
    for label, exe, flags in variants:
        out = os.path.join(tmp, "out_%d_%d" % (r, len(profiles))) + "/"
        os.makedirs(out, exist_ok=True)
        t0 = time.time()
        p = subprocess.run([exe] + flags + ["-w", "1000", "-o", out, db, bam], capture_output=True, text=True, env=dict(os.environ, SLIMM_TRACE="cli"))
        dt = time.time() - t0
        if p.returncode != 0:
            print(f"   {label}: FAILED {p.stderr[-400:]}", flush=True)
            sys.exit(1)
        profiles.setdefault(label, open(os.path.join(out, "realistic_profile.tsv")).read())
        if r == 0:
            continue
        times[label].append(dt)
        if label not in best or dt < best[label][0]:
            best[label] = (dt, "\n".join("      " + l[l.index("[trace]"):] for l in p.stderr.splitlines() if "[trace]" in l),
                           "\n".join("      " + l.strip() for l in p.stderr.splitlines() if "record filter:" in l))
for label, _, _ in variants:
    t = times[label]
    print(f"   slimm DB realistic.bam [{label}]: " + " ".join("%.3f" % x for x in t) + f" s; best {min(t):.3f} s = {n / min(t) / 1e6:.1f} M records/s\n"
          + best[label][2] + "\n" + best[label][1], flush=True)
print("   profiles equal: no option = -q/-F variant: %s; no option = aligned/identity variant: %s%s" % (
    profiles["no option"] == profiles["-q 10 --exclude-flags 0xF00"], profiles["no option"] == profiles["--min-aligned 50 --min-identity 0.95"],
    ("; other build = no option: %s" % (profiles["other build, no option"] == profiles["no option"])) if "other build, no option" in profiles else ""))
