#!/bin/bash
# rocprofv3 kernel stats of tools/profile/dither_cost.py: usage dither_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/dither_cost.json (ms per NES step, dither 0 / 1 on both MFCC routes) and kernel_stats.csv
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t1" -o p -- python tools/profile/dither_cost.py "$@" > "$O/dither_cost.json" || exit $?
cp "$(find "$O/t1" -name "*kernel_stats.csv" | head -1)" "$O/kernel_stats.csv" && rm -rf "$O/t1"
python - "$O/kernel_stats.csv" <<'PY'
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    if "mfcc" in r["Name"]:
        print("%-90s calls %5s avg %9.1f ns" % (r["Name"][:90], r["Calls"], float(r["AverageNs"])))
PY
cat "$O/dither_cost.json"
