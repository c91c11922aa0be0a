#!/bin/bash
# rocprofv3 kernel trace of tools/profile/air_channel_cost.py: usage air_channel_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/air_channel_cost.json (ms per NES step of each run, untraced) and air_kernel_times.json: the solo time of
# k_air_conv at L = 512, 2048, 4096 over the 51 x 48 000 batch with its time per (sample * tap) and its useful-flop share of
# the f64 MFMA peak, the 511-tap FIR stage of k_input_transform over the same batch as the yardstick, and the mean times of
# k_air_taps / k_air_conv inside the NES runs -- all from the trace
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
# step times with the profiler off, then the kernels' own times in a traced run of the same program
timeout -k 10 240 python tools/profile/air_channel_cost.py "$@" > "$O/air_channel_cost.json" &&
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t1" -o p -- python tools/profile/air_channel_cost.py "$@" > "$O/traced_run.json" || exit $?
python - "$(find "$O/t1" -name "*kernel_trace.csv" | head -1)" "$O/traced_run.json" > "$O/air_kernel_times.json" <<'PY'
import csv, json, sys
run = json.load(open(sys.argv[2]))
trace = list(csv.DictReader(open(sys.argv[1])))
PEAK = 78.6e12   # f64 MFMA, flop / s
def times(kern):
    return [b - a for a, b in sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in trace if kern in r["Kernel_Name"])]
def stat(d):
    return dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d))
reps, cells = run["hook_reps"], run["rows"] * run["samples"]
conv, fir, taps = times("k_air_conv"), times("k_input_transform"), times("k_air_taps")
out = {}
for i, L in enumerate(run["hook_taps"]):
    s = stat(conv[i * reps + 1:(i + 1) * reps])   # (the first call of each size left out)
    s["ps_per_sample_tap"] = s["mean_us"] * 1e6 / (cells * L)
    s["useful_flop_share_of_peak"] = 2.0 * cells * L / (s["mean_us"] * 1e-6) / PEAK
    out["k_air_conv L=%d" % L] = s
s = stat(fir[1:reps])
s["ps_per_sample_tap"] = s["mean_us"] * 1e6 / (cells * 511)
out["k_input_transform fir511"] = s
per = run["steps"] + run["warmup"]
nes_conv, nes_taps = conv[len(run["hook_taps"]) * reps:], taps
air_runs = [n for n in run["order"] if n.startswith("air")]
if len(nes_conv) == per * len(air_runs) == len(nes_taps):
    for i, n in enumerate(air_runs):   # the timed steps of run i (its warm-up dispatches left out)
        out[n] = {"k_air_conv": stat(nes_conv[i * per + run["warmup"]:(i + 1) * per]), "k_air_taps": stat(nes_taps[i * per + run["warmup"]:(i + 1) * per])}
else:                              # (another dispatch count than one per step: the runs cannot be told apart)
    out["air runs together"] = {"k_air_conv": stat(nes_conv), "k_air_taps": stat(nes_taps)}
print(json.dumps(out))
PY
rm -rf "$O/t1" "$O/traced_run.json"
cat "$O/air_channel_cost.json" "$O/air_kernel_times.json"
