#!/bin/bash
# rocprofv3 kernel trace of tools/profile/codec_cost.py: usage codec_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/codec_cost.json (ms per NES step of each run, untraced) and codec_kernel_times.json: the solo time of
# k_codec per kind over the 51 x 48 000 batch and over 204 x 48 000, with its time per sample, and the mean time of k_codec
# inside each NES run -- all from the trace (a kernel trace only: no counters in the same run)
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
# step times with the profiler off, then the kernels' own times in a traced run of the same program
timeout -k 10 240 python tools/profile/codec_cost.py "$@" > "$O/codec_cost.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t1" -o p -- python tools/profile/codec_cost.py "$@" > "$O/traced_run.json" || exit $?
python - "$(find "$O/t1" -name "*kernel_trace.csv" | head -1)" "$O/traced_run.json" > "$O/codec_kernel_times.json" <<'PY'
import csv, json, sys
run = json.load(open(sys.argv[2]))
trace = list(csv.DictReader(open(sys.argv[1])))
def times(kern):
    return [b - a for a, b in sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in trace if kern in r["Kernel_Name"])]
def stat(d):
    return dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d))
reps, kinds = run["hook_reps"], run["hook_kinds"]
codec = times("k_codec")
out, i = {}, 0
for rows in run["hook_rows"]:
    for kind in kinds:
        s = stat(codec[i + 1:i + reps])   # (the first call of each shape left out)
        s["ps_per_sample"] = s["mean_us"] * 1e6 / (rows * run["samples"])
        s["ns_per_sample_of_a_row"] = s["mean_us"] * 1e3 / run["samples"]
        out["k_codec %s %d rows" % (kind, rows)] = s
        i += reps
per = run["steps"] + run["warmup"]
nes = codec[i:]
coded = [n for n in run["order"] if not n.startswith("none")]
if len(nes) == per * len(coded):
    for j, n in enumerate(coded):   # the timed steps of run j (its warm-up dispatches left out)
        out[n] = {"k_codec": stat(nes[j * per + run["warmup"]:(j + 1) * per])}
else:                               # (another dispatch count than one per step: the runs cannot be told apart)
    out["coded runs together"] = {"k_codec": stat(nes), "expected_dispatches": per * len(coded)}
print(json.dumps(out))
PY
rm -rf "$O/t1" "$O/traced_run.json"
cat "$O/codec_cost.json" "$O/codec_kernel_times.json"
