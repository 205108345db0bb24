"""python profiles/pmc_sum.py <dir> <tag>: per sweep stage, mean counter value per launch / mean kernel time, from rocprofv3 csv output."""
import collections, csv, glob, os, re, sys
d, tag = sys.argv[1:3]
agg = collections.defaultdict(list)
for f in glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        m = re.search(r"sweep_kernel<.*?,\s*(\d+)>", r["Kernel_Name"])
        if m:
            agg[(r["Counter_Name"], int(m.group(1)))].append(float(r["Counter_Value"]))
for (c, s), v in sorted(agg.items()):
    print(tag, c, "stage", s, "launches", len(v), "mean", sum(v) / len(v))
for f in glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        m = re.search(r"sweep_kernel<.*?,\s*(\d+)>", r["Name"])
        if m:
            print(tag, "kernel_stats stage", m.group(1), "calls", r["Calls"], "avg_ns", r["AverageNs"], "min_ns", r["MinNs"], "max_ns", r["MaxNs"])
