"""How k_update_perturb meets the other attacks' k_gmm_fx2w launches on a shared GPU, from a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o p -- python bench.py --full --no-cpu-baseline --no-secondary
    python tools/profile/update_shape_trace.py <dir>/.../p_kernel_trace.csv

For every k_update_perturb dispatch: how many k_gmm_fx2w dispatches of OTHER streams were running when it started, and the
dispatch's duration by that count; then every kernel's calls, average, minimum and maximum (profiles/update_shape_*)."""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
ev = []
for r in rows:
    name = r["Kernel_Name"].split("(")[0].replace("void ", "")
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, r.get("Stream_Id") or r.get("Queue_Id")))
ev.sort()
fx = [e for e in ev if e[2].startswith("k_gmm_fx2w")]
up = [e for e in ev if e[2].startswith("k_update_perturb")]
hist = collections.Counter()
dur = collections.defaultdict(list)
for s, e, n, q in up:
    k = sum(1 for fs, fe, _, fq in fx if fs <= s < fe and fq != q)
    hist[k] += 1
    dur[k].append((e - s) / 1e3)
print("k_update_perturb dispatches: %d" % len(up))
for k in sorted(hist):
    d = sorted(dur[k])
    print("  starts while %d k_gmm_fx2w of other streams run: %d (%.1f %%), duration avg %.1f us, median %.1f, min %.1f, max %.1f" %
          (k, hist[k], 100.0 * hist[k] / len(up), sum(d) / len(d), d[len(d) // 2], d[0], d[-1]))
by = collections.defaultdict(list)
for s, e, n, q in ev:
    by[n].append((e - s) / 1e3)
print("kernel, calls, avg us, min us, max us")
for n, d in sorted(by.items(), key=lambda x: -sum(x[1])):
    print("  %s, %d, %.1f, %.1f, %.1f" % (n, len(d), sum(d) / len(d), min(d), max(d)))
