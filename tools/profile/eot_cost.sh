#!/bin/bash
# rocprofv3 kernel trace of tools/profile/eot_cost.py: usage eot_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/eot_cost.json (ms per NES step of each run, untraced), eot_kernel_times.json (mean time of
# k_input_transform, k_tf_power and k_loss_eot per run, from the trace) and kernel_stats.csv
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
# step times with the profiler off, then the kernels' own times in a traced run of the same program
timeout -k 10 240 python tools/profile/eot_cost.py "$@" > "$O/eot_cost.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t1" -o p -- python tools/profile/eot_cost.py "$@" > "$O/traced_run.json" || exit $?
cp "$(find "$O/t1" -name "*kernel_stats.csv" | head -1)" "$O/kernel_stats.csv" || exit 1
python - "$(find "$O/t1" -name "*kernel_trace.csv" | head -1)" "$O/traced_run.json" > "$O/eot_kernel_times.json" <<'PY'
import csv, json, sys
run = json.load(open(sys.argv[2]))
per = run["steps"] + run["warmup"]
trace = list(csv.DictReader(open(sys.argv[1])))
out = {}
for kern, runs in (("k_input_transform", [n for n in run["order"] if not n.startswith("none") and n != "dither 1 r=1"]),
                   ("k_tf_power", [n for n in run["order"] if n.startswith("at:")]),
                   ("k_loss_eot", [n for n in run["order"] if not n.endswith("r=1") and not n.endswith("again")])):
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in trace if kern in r["Kernel_Name"])
    assert len(rows) == per * len(runs), (kern, len(rows), per, runs)
    for i, n in enumerate(runs):   # the timed steps of run i (its warm-up dispatches left out)
        d = [b - a for a, b in rows[i * per + run["warmup"]:(i + 1) * per]]
        out.setdefault(n, {})[kern] = dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d))
print(json.dumps(out))
PY
rm -rf "$O/t1" "$O/traced_run.json"
cat "$O/eot_cost.json" "$O/eot_kernel_times.json"
