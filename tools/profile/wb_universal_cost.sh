#!/bin/bash
# the cost of white-box gradients of a universal perturbation: usage wb_universal_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/wb_universal_cost.json (tools/profile/wb_universal_cost.py all: ms per fb_attack_wb iteration, untraced) and
# wb_universal_kernel_times.json: from a rocprofv3 kernel trace of `wb_universal_cost.py hook` in a run of its own, the time of
# k_wb_compose_t at N = 48 000 for R = 8 and R = 32 (the launches in the order run) against its byte count
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
timeout -k 10 420 python tools/profile/wb_universal_cost.py all "$@" > "$O/wb_universal_cost.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -o p -- python tools/profile/wb_universal_cost.py hook 30 0 > "$O/traced_run.json" || exit $?
python - "$O" > "$O/wb_universal_kernel_times.json" <<'PY'
import csv, glob, json, os, sys
O = sys.argv[1]
run = json.load(open(os.path.join(O, "traced_run.json")))
per, n = run["steps"], run["samples"]
trace = list(csv.DictReader(open(glob.glob(os.path.join(O, "trace", "**", "*kernel_trace.csv"), recursive=True)[0])))
d = [b - a for a, b in sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in trace if r["Kernel_Name"].startswith("k_wb_compose_t"))]
def stat(d, R, K):
    d = sorted(d)
    nbytes = n * (R * 8 + (K + 1) * 2 + 8)
    med = d[len(d) // 2]
    return dict(median_us=med / 1e3, min_us=d[0] / 1e3, max_us=d[-1] / 1e3, dispatches=len(d), bytes=nbytes, gb_per_s_at_median=nbytes / med)
print(json.dumps({"k_wb_compose_t R=8 (K=4, eot=2)": stat(d[1:per], 8, 4), "k_wb_compose_t R=32 (K=32, eot=1)": stat(d[per + 1:2 * per], 32, 32),
                  "dispatches": len(d)}))
PY
rm -rf "$O/trace" "$O/traced_run.json"
cat "$O/wb_universal_cost.json" "$O/wb_universal_kernel_times.json"
