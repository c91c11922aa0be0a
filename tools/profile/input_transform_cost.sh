#!/bin/bash
# rocprofv3 kernel trace of tools/profile/input_transform_cost.py: usage input_transform_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/input_transform_cost.json (ms per NES step without a chain and with each chain, untraced run),
# input_transform_kernel_times.json (k_input_transform's mean time per chain, from the trace) and kernel_stats.csv
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
# step times with the profiler off, then the kernels' own times in a traced run of the same program
timeout -k 10 240 python tools/profile/input_transform_cost.py "$@" > "$O/input_transform_cost.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t1" -o p -- python tools/profile/input_transform_cost.py "$@" > "$O/traced_run.json" || exit $?
cp "$(find "$O/t1" -name "*kernel_stats.csv" | head -1)" "$O/kernel_stats.csv" || exit 1
python - "$(find "$O/t1" -name "*kernel_trace.csv" | head -1)" "$O/traced_run.json" > "$O/input_transform_kernel_times.json" <<'PY'
import csv, json, sys
run = json.load(open(sys.argv[2]))
per = run["steps"] + run["warmup"]
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(sys.argv[1]))
              if "k_input_transform" in r["Kernel_Name"])
names = [n for n in run["order"] if not n.startswith("none")]
assert len(rows) == per * len(names), (len(rows), per, names)
out = {}
for i, n in enumerate(names):   # the timed steps of chain i (its warm-up dispatches left out)
    d = [b - a for a, b in rows[i * per + run["warmup"]:(i + 1) * per]]
    out[n] = dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d))
print(json.dumps(out))
PY
rm -rf "$O/t1" "$O/traced_run.json"
cat "$O/input_transform_cost.json" "$O/input_transform_kernel_times.json"
