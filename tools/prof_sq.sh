#!/bin/bash
# SQ counters of the full bench's kernels (one --pmc pass, 8 SQ slots): tools/prof_sq.sh TAG [bench args...]
# (results in $OUT, default prof_out/ in the repository root)
set -e
TAG=$1; shift
cd "$(dirname "$0")/.."
OUT=${OUT:-prof_out}
PROF=$(mktemp -d)
mkdir -p "$OUT"
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS \
  --output-format csv -d "$PROF" -o sq -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" > /dev/null 2> "$OUT/${TAG}_sq.err"
python3 - "$TAG" "$PROF" "$OUT" <<'PY'
import csv, glob, sys, collections
tag, prof, out = sys.argv[1:4]
f = glob.glob(prof + "/**/*counter_collection.csv", recursive=True)[0]
per = collections.defaultdict(lambda: collections.defaultdict(list))
for r in csv.DictReader(open(f)):
    per[r["Kernel_Name"][:60]][r["Counter_Name"].replace("SQ_", "")].append(float(r["Counter_Value"]))
with open(f"{out}/{tag}_sq.txt", "w") as o:
    for k, c in per.items():
        if "ga::" not in k: continue
        m = {n: sum(v) / len(v) for n, v in c.items()}
        wc = m.get("WAVE_CYCLES", 1)
        line = f"{k:60s} launches {len(c['WAVE_CYCLES']):3d} wave_cycles {wc:.3e} " + " ".join(f"{n} {v / wc:.2f}" for n, v in m.items() if n != "WAVE_CYCLES")
        print(line); o.write(line + "\n")
PY
rm -rf "$PROF"
