#!/bin/bash
# timeline of one headline bench run: kernels + memory copies (no counters), gaps between consecutive device activities
# tools/trace_gaps.sh TAG [bench args...]   (results in $OUT, default prof_out/ in the repository root)
set -e
TAG=$1; shift
cd "$(dirname "$0")/.."
OUT=${OUT:-prof_out}
PROF=$(mktemp -d)
mkdir -p "$OUT"
rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d "$PROF" -o t -- python3 bench.py --steps 6 --warmup 2 "$@" > /dev/null 2> "$OUT/${TAG}_trace.err"
python3 - "$TAG" "$PROF" "$OUT" <<'PY'
import csv, glob, sys
tag, prof, out = sys.argv[1:4]
ev = []
for f in glob.glob(prof + "/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "K " + r["Kernel_Name"][:40]))
for f in glob.glob(prof + "/**/*memory_copy_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "C " + r.get("Direction", r.get("Kind", "?")) ))
ev.sort()
t0 = ev[0][0]
with open(f"{out}/{tag}_trace.txt", "w") as o:
    last_end = None
    for s, e, n in ev[-90:]:
        gap = (s - last_end) / 1e3 if last_end else 0.0
        line = f"{(s - t0) / 1e6:10.3f} ms  dur {(e - s) / 1e3:9.1f} us  gap {gap:8.1f} us  {n}"
        print(line); o.write(line + "\n")
        last_end = max(last_end or 0, e)
PY
rm -rf "$PROF"
