#!/bin/bash
# Counters of the gate/up decode GEMM (8 rows, cold weights) on the 13-bit image and on the bf16 image: bytes fetched, VALU busy,
# occupancy.  One rocprofv3 pass per counter with --pmc and NO tracing flag; per kernel averages -> <out>.  A pass that ends with ANY
# non-zero status ends the script: nothing more is started on the card after trouble.
# usage (on the GPU box, from the repository root): bash tools/z13_pmc.sh <out.txt>
OUT=${1:-z13_gate_up_pmc.txt}
export TMPDIR=/tmp
W=$(mktemp -d)
: > "$OUT"
for C in FETCH_SIZE VALUBusy MeanOccupancyPerCU; do
  D=$W/$C
  mkdir -p "$D"
  timeout -k 10 150 rocprofv3 --pmc $C --output-format csv -d "$D" -o pmc -- python tools/z13_decode_bench.py --legs pmc > "$D/log.txt" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then
    echo "pass $C ended with status $rc: stopping" | tee -a "$OUT"
    tail -5 "$D/log.txt" | tee -a "$OUT"
    rm -rf "$W"
    exit $rc
  fi
  python - "$D" "$C" >> "$OUT" <<'PY' || { rm -rf "$W"; exit 1; }
import collections, csv, glob, sys
d, c = sys.argv[1], sys.argv[2]
files = glob.glob(d + "/**/*counter_collection.csv", recursive=True)
if not files:
    print(f"{c}: no counter file")
    sys.exit(0)
acc = collections.defaultdict(list)
for r in csv.DictReader(open(files[0])):
    k = r.get("Kernel_Name", "")
    if "gemm_skinny" in k:
        acc[(r.get("Counter_Name"), k[:90])].append(float(r.get("Counter_Value", "nan")))
for (n, k), v in sorted(acc.items()):
    print(f"{n:20s} {k:90s} n={len(v):4d} avg={sum(v) / len(v):.6g}")
PY
done
rm -rf "$W"
cat "$OUT"
