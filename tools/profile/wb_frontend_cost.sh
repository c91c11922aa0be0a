#!/bin/bash
# the cost of white-box gradients through feature compression and dither: usage wb_frontend_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/wb_frontend_cost.json (tools/profile/wb_frontend_cost.py all: ms per fb_attack_wb iteration, untraced) and
# wb_frontend_kernel_times.json: from a rocprofv3 kernel trace of `wb_frontend_cost.py trace` in a run of its own, the mean time
# of k_wb_mfcc_t without and with dither 1.0 (the launches in the order run: no stage, dither, FeCo), of k_feature_compress with
# the keep outputs on and of k_wb_feco_t
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
timeout -k 10 420 python tools/profile/wb_frontend_cost.py all "$@" > "$O/wb_frontend_cost.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/trace" -o p -- python tools/profile/wb_frontend_cost.py trace 20 4 > "$O/traced_run.json" || exit $?
python - "$O" > "$O/wb_frontend_kernel_times.json" <<'PY'
import csv, glob, json, os, sys
O = sys.argv[1]
run = json.load(open(os.path.join(O, "traced_run.json")))
per = run["steps"] + run["warmup"]
trace = list(csv.DictReader(open(glob.glob(os.path.join(O, "trace", "**", "*kernel_trace.csv"), recursive=True)[0])))
def times(name):
    return [b - a for a, b in sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in trace if r["Kernel_Name"].startswith(name))]
def stat(d):
    return dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d)) if d else None
m = times("k_wb_mfcc_t")
out = {"k_wb_mfcc_t no dither": stat(m[1:per]), "k_wb_mfcc_t dither 1.0": stat(m[per + 1:2 * per]), "k_wb_mfcc_t under FeCo": stat(m[2 * per + 1:3 * per]),
       "k_wb_mfcc_t dispatches": len(m), "k_feature_compress (keep on)": stat(times("k_feature_compress")[1:]), "k_wb_feco_t": stat(times("k_wb_feco_t")[1:])}
print(json.dumps(out))
PY
rm -rf "$O/trace" "$O/traced_run.json"
cat "$O/wb_frontend_cost.json" "$O/wb_frontend_kernel_times.json"
