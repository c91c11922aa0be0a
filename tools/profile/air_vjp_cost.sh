#!/bin/bash
# rocprofv3 kernel trace of tools/profile/air_vjp_cost.py: usage air_vjp_cost.sh <output dir> [steps [warmup]]
# writes <output dir>/air_vjp_cost.json (ms per fb_attack_wb iteration at eot 8 without and through a 2048-tap channel, untraced)
# and air_vjp_kernel_times.json: the solo times of k_air_conv (the yardstick) and k_air_conv_t at 8 and 32 rows x 48 000 samples,
# L = 512, 2048, 4096, with the time per (sample * tap) and the transpose's ratio to the forward; the 8 rows at L = 2048 as
# eight one-row launches (summed) against the one batched launch; and k_air_conv_t at L = 2048 in the 16- and 17-slot LDS
# layouts (FB_AIRT_PAD) -- all from kernel traces, each in a run of its own
set -o pipefail
R=$(cd "$(dirname "$0")/../.." && pwd); O=$1; shift; mkdir -p "$O"; O=$(cd "$O" && pwd)
cd "$R" || exit 1
export PYTHONPATH=$R TMPDIR=/tmp
timeout -k 10 240 python tools/profile/air_vjp_cost.py all "$@" > "$O/air_vjp_cost.json" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t18" -o p -- python tools/profile/air_vjp_cost.py hooks > "$O/traced_run.json" &&
FB_AIRT_PAD=17 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t17" -o p -- python tools/profile/air_vjp_cost.py hooks > /dev/null &&
FB_AIRT_PAD=16 timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/t16" -o p -- python tools/profile/air_vjp_cost.py hooks > /dev/null || exit $?
python - "$O" > "$O/air_vjp_kernel_times.json" <<'PY'
import csv, glob, json, os, sys
O = sys.argv[1]
run = json.load(open(os.path.join(O, "traced_run.json")))
reps, taps, rows_list, samples = run["hook_reps"], run["hook_taps"], run["rows"], run["samples"]
def load(d):
    trace = list(csv.DictReader(open(glob.glob(os.path.join(O, d, "**", "*kernel_trace.csv"), recursive=True)[0])))
    def times(pred):
        return [b - a for a, b in sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in trace if pred(r["Kernel_Name"]))]
    return times(lambda k: "k_air_conv" in k and "k_air_conv_t" not in k), times(lambda k: "k_air_conv_t" in k)
def stat(d):
    return dict(mean_us=sum(d) / len(d) / 1e3, min_us=min(d) / 1e3, max_us=max(d) / 1e3, dispatches=len(d))
out = {}
for pad in (18, 17, 16):
    fwd, tr = load("t%d" % pad)
    i = 0
    for rows in rows_list:
        for L in taps:
            f, t = stat(fwd[i * reps + 1:(i + 1) * reps]), stat(tr[i * reps + 1:(i + 1) * reps])   # (the first call of each size left out)
            cells = rows * samples * L
            f["ps_per_sample_tap"], t["ps_per_sample_tap"] = f["mean_us"] * 1e6 / cells, t["mean_us"] * 1e6 / cells
            t["ratio_to_forward"] = t["mean_us"] / f["mean_us"]
            if pad == 18:
                out["k_air_conv rows=%d L=%d" % (rows, L)] = f
            out["k_air_conv_t pad=%d rows=%d L=%d" % (pad, rows, L)] = t
            i += 1
    single = tr[i * reps:]                  # reps x 8 one-row launches
    per_call = [sum(single[c * 8:(c + 1) * 8]) for c in range(1, reps)]
    out["k_air_conv_t pad=%d eight one-row launches L=2048, kernel time summed" % pad] = stat(per_call)
print(json.dumps(out))
PY
rm -rf "$O/t18" "$O/t17" "$O/t16" "$O/traced_run.json"
cat "$O/air_vjp_cost.json" "$O/air_vjp_kernel_times.json"
