#!/bin/bash
# A/B of two checkouts on one box: the headline bench of this tree and of another built tree (its own Python layer and
# library: an older library lacks entry points a newer binding asks for), alternated round by round.
# (tools/ab_lib.sh, which alternated two LIBRARIES under one Python layer, left the tree with the lab scripts of rounds
#  4 - 5; tools/ab_exact.sh still does that for SCARPLET_HIP_LIB builds that share this tree's ABI entries.)
#   tools/ab_tree.sh <other tree> <rounds> <out dir> [bench arguments ...]
# Writes <out dir>/{this,other}_<round>.json (the bench's result line) and prints step time and kernels_ms_per_step.
# A run that fails or overruns its time limit ends the script: nothing more is started on the GPU after it.
OTHER=$1; ROUNDS=$2; OUT=$3; shift 3
HERE=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$OUT"
for r in $(seq 1 "$ROUNDS"); do
  for side in other this; do
    tree=$HERE; [ $side = other ] && tree=$OTHER
    timeout -k 10 300 python3 "$tree/bench.py" --gpus 1 "$@" > "$OUT/${side}_$r.log" 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then echo "$side round $r: exit status $rc"; tail -5 "$OUT/${side}_$r.log"; exit $rc; fi
    grep '^{' "$OUT/${side}_$r.log" | tail -1 > "$OUT/${side}_$r.json"
    python3 - "$OUT/${side}_$r.json" $side $r <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
k = d.get("kernels_ms_per_step", {})
print("%-5s round %s: step %.2f ms  kernels %.1f ms %s  %s MHz  build %s" % (sys.argv[2], sys.argv[3], d["ms_per_step"], sum(k.values()),
      json.dumps(k, sort_keys=True), d.get("gpu", {}).get("clock_mhz", "?"), d["library"]["build_id"]))
PY
  done
done
