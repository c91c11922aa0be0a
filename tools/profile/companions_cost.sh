#!/bin/bash
# rocprofv3 kernel trace of tools/profile/companions_cost.py: usage companions_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/companions_cost.json (ms per NES step of each run, untraced), companions_kernel_times.json (mean time
# of k_input_transform_cmp, k_tf_power_cmp and k_loss_eot per run, from the trace) and kernel_stats.csv
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
# step times with the profiler off, then the kernels' own times in a traced run of the same program
timeout -k 10 240 python tools/profile/companions_cost.py "$@" > "$O/companions_cost.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t1" -o p -- python tools/profile/companions_cost.py "$@" > "$O/traced_run.json" || exit $?
cp "$(find "$O/t1" -name "*kernel_stats.csv" | head -1)" "$O/kernel_stats.csv" || exit 1
python - "$(find "$O/t1" -name "*kernel_trace.csv" | head -1)" "$O/traced_run.json" > "$O/companions_kernel_times.json" <<'PY'
import csv, json, sys
run = json.load(open(sys.argv[2]))
per = run["steps"] + run["warmup"]
trace = list(csv.DictReader(open(sys.argv[1])))
multi = [n for n in run["order"] if "K=1" not in n]
out = {}
for kern, runs in (("k_input_transform_cmp", multi), ("k_tf_power_cmp", [n for n in multi if n.startswith("at:")]), ("k_loss_eot", multi)):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in trace if kern in r["Kernel_Name"])
    assert len(rows) == per * len(runs), (kern, len(rows), per, runs)
    for i, n in enumerate(runs):   # the timed steps of run i (its warm-up dispatches left out)
        d = [b - a for a, b in rows[i * per + run["warmup"]:(i + 1) * per]]
        out.setdefault(n, {})[kern] = dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d))
print(json.dumps(out))
PY
rm -rf "$O/t1" "$O/traced_run.json"
cat "$O/companions_cost.json" "$O/companions_kernel_times.json"
