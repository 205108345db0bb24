"""python profiles/ab_table.py <ab_runs.txt>: the markdown table of an ab_forms.sh job, in run order, and per form the spread of
each tree, the median gain and whether every new `value` is above every parent `value` (the test of r7_valu_diet.md section 3)."""
import json
import statistics
import sys

runs = []
for line in open(sys.argv[1]):
    tree, form, js = line.split(" ", 2)
    runs.append((tree, form, json.loads(js)))
print("| # | tree | form | value (particle-steps/s) | ms/step | steady_state ms/step | B / C / D µs (events) | placement |")
print("|---|---|---|---|---|---|---|---|")
for n, (tree, form, d) in enumerate(runs, 1):
    k = d["kernels"]
    us = " / ".join("%.1f" % (k[s]["avg_ms"] * 1e3) for s in ("sweep_B", "sweep_C", "sweep_D") if s in k)
    print("| %d | %s | %s | %.4e | %.4f | %.4f | %s | %s |" % (n, tree, form, d["value"], d["ms_per_step"],
                                                            d.get("steady_state", {}).get("ms_per_step", float("nan")), us,
                                                            d["placement"]["outcome"]))
print()
for form in ("default", "short"):
    v = {t: [d["value"] for tree, f, d in runs if tree == t and f == form] for t in ("parent", "new")}
    if not v["parent"] or not v["new"]:
        continue
    spread = {t: (max(x) - min(x)) / statistics.median(x) * 100 for t, x in v.items()}
    gain = (statistics.median(v["new"]) / statistics.median(v["parent"]) - 1) * 100
    print("%s: parent %.4e–%.4e (spread %.2f %%), new %.4e–%.4e (spread %.2f %%), median gain %+.2f %% = %.1f x the larger spread, "
          "every new above every parent: %s" % (form, min(v["parent"]), max(v["parent"]), spread["parent"], min(v["new"]), max(v["new"]),
                                                spread["new"], gain, gain / max(spread.values()),
                                                "yes" if min(v["new"]) > max(v["parent"]) else "NO"))
    print()
