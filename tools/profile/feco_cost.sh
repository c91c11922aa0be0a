#!/bin/bash
# rocprofv3 kernel trace of tools/profile/feco_cost.py: usage feco_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/feco_cost.json: the ms per NES step of each run (untraced) and, under "kernel", the mean time of
# k_feature_compress per run (from the trace); and kernel_stats.csv
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
# step times with the profiler off, then the kernel's own times in a traced run of the same program
timeout -k 10 240 python tools/profile/feco_cost.py "$@" > "$O/steps.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t1" -o p -- python tools/profile/feco_cost.py "$@" > "$O/traced_run.json" || exit $?
cp "$(find "$O/t1" -name "*kernel_stats.csv" | head -1)" "$O/kernel_stats.csv" || exit 1
python - "$(find "$O/t1" -name "*kernel_trace.csv" | head -1)" "$O/traced_run.json" "$O/steps.json" > "$O/feco_cost.json" <<'PY'
import csv, json, sys
run = json.load(open(sys.argv[2]))
out = json.load(open(sys.argv[3]))
per = run["steps"] + run["warmup"]
runs = [n for n in run["order"] if n.startswith("feco")]
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(sys.argv[1]))
              if "k_feature_compress" in r["Kernel_Name"])
assert len(rows) == per * len(runs), (len(rows), per, runs)
out["kernel"] = {}
for i, n in enumerate(runs):   # the timed steps of run i (its warm-up dispatches left out)
    d = [b - a for a, b in rows[i * per + run["warmup"]:(i + 1) * per]]
    out["kernel"][n] = dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d))
print(json.dumps(out))
PY
rm -rf "$O/t1" "$O/traced_run.json" "$O/steps.json"
cat "$O/feco_cost.json"
