#!/bin/bash
# per-kernel times of the full bench (headline + variants) under rocprofv3: tools/kstats.sh TAG
# (results in $OUT, default prof_out/ in the repository root)
cd "$(dirname "$0")/.."
TAG=${1:-ks}
OUT=${OUT:-prof_out}
PROF=$(mktemp -d)
mkdir -p "$OUT"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$PROF" -o st -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > "$OUT/${TAG}_bench.json" 2> "$OUT/${TAG}.err"
cp "$(find "$PROF" -name "*kernel_stats.csv" | head -1)" "$OUT/${TAG}_kernel_stats.csv"
rm -rf "$PROF"
python3 - "$OUT/${TAG}_kernel_stats.csv" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if float(r["TotalDurationNs"]) > 2e5: print(f'{r["Name"][:60]:60s} calls {r["Calls"]:>5s} avg {float(r["AverageNs"])/1e6:8.3f} ms')
PY
