#!/bin/bash
# k_filter_compact, another build of the library against this tree's, ALTERNATED in one call on one MI355X:
#   scripts/filter_ab.sh OTHER_LIB [kernel|headline|configs|outputs|counters ...]     (default: all five, in that order)
# OTHER_LIB = the other libslimm_hip.so (the parent's: `git archive` of it, make -C slimm_amd/csrc ../libslimm_hip.so).
#   kernel    python bench.py --breakdown, three pairs: the k_filter line of each
#   headline  plain python bench.py, five pairs: ms per step of each, medians, the other build's spread
#   configs   --config config2 / config3 / config5 --breakdown, two pairs each
#   outputs   --dump-outputs of both: every .npy byte for byte, profile_sha1
#   counters  scripts/pmc_sq.sh of both (counters in runs of their own): the k_filter_compact lines
# Everything lands in $FILTER_AB_OUT (default: filter_ab_out/, kept out of git); every step has
# its own time limit and a failure ends the script.
set -o pipefail
OTHER=$(readlink -f "$1"); shift
[ -f "$OTHER" ] || { echo "usage: $0 OTHER_LIB [legs]"; exit 2; }
LEGS=${*:-kernel headline configs outputs counters}
O=${FILTER_AB_OUT:-filter_ab_out}; mkdir -p $O
use() { if [ $1 = this ]; then unset SLIMM_HIP_LIB; else export SLIMM_HIP_LIB=$OTHER; fi; }
bench() {  # tag build args...
  local tag=$1 b=$2; shift 2
  use $b
  timeout -k 10 300 python bench.py "$@" > $O/$tag.json 2> $O/$tag.txt || { echo "FAILED $tag"; tail -20 $O/$tag.txt; exit 1; }
}
field() { python3 -c "import json,sys; print(json.loads(open(sys.argv[1]).read().strip().split('\n')[-1]).get(sys.argv[2]))" $O/$1.json $2; }
for leg in $LEGS; do
  case $leg in
  kernel)
    for rep in 1 2 3; do for b in other this; do
      bench bd_${b}_$rep $b --breakdown --steps 10 --warmup 3
      echo "kernel $b $rep $(grep -E '^# k_filter ' $O/bd_${b}_$rep.txt) | $(grep -E '^# device kernels' $O/bd_${b}_$rep.txt)"
    done; done ;;
  headline)
    for rep in 1 2 3 4 5; do for b in other this; do
      bench plain_${b}_$rep $b
      echo "headline $b $rep $(field plain_${b}_$rep ms_per_step) ms per step"
    done; done
    python3 - $O <<'PY'
import json, statistics, sys
ms = {b: [json.loads(open(f"{sys.argv[1]}/plain_{b}_{r}.json").read().strip().split("\n")[-1])["ms_per_step"] for r in range(1, 6)] for b in ("other", "this")}
for b in ms: print(f"  {b:6s}", *ms[b], f"  median {statistics.median(ms[b]):.4f}  max - min {max(ms[b]) - min(ms[b]):.4f}")
gain = statistics.median(ms["other"]) - statistics.median(ms["this"])
print(f"  gain of the medians {gain:.4f} ms; slowest of this build {max(ms['this'])} against fastest of the other {min(ms['other'])}: "
      + ("every run of this build is faster" if max(ms["this"]) < min(ms["other"]) else "NOT every run of this build is faster"))
PY
    ;;
  configs)
    for c in config2 config3 config5; do for rep in 1 2; do for b in other this; do
      bench ${c}_${b}_$rep $b --config $c --breakdown --steps 10 --warmup 3
      echo "$c $b $rep $(grep -E '^# k_filter ' $O/${c}_${b}_$rep.txt) | $(grep -E '^# device kernels' $O/${c}_${b}_$rep.txt)"
    done; done; done ;;
  outputs)
    for b in other this; do
      rm -rf $O/dump_$b; bench dump_$b $b --steps 2 --warmup 1 --dump-outputs $O/dump_$b
      (cd $O/dump_$b && sha1sum *.npy) > $O/dump_$b.sha1; rm -rf $O/dump_$b
      echo "outputs $b profile_sha1 $(field dump_$b profile_sha1)"
    done
    if cmp -s $O/dump_other.sha1 $O/dump_this.sha1; then echo "outputs: $(wc -l < $O/dump_this.sha1) .npy files byte-identical"
    else echo "OUTPUTS DIFFER"; diff $O/dump_other.sha1 $O/dump_this.sha1; exit 1; fi ;;
  counters)
    for b in other this; do
      use $b
      timeout -k 10 400 bash scripts/pmc_sq.sh filter_ab/sq_$b > $O/sq_$b.txt 2>&1 || { echo "FAILED counters $b"; tail -20 $O/sq_$b.txt; exit 1; }
      echo "counters $b $(grep k_filter_compact $O/sq_$b.txt)"
    done ;;
  *) echo "unknown leg $leg"; exit 2 ;;
  esac
done
