"""Compare two rocprofv3 output directories of profiles/plan_refactor_trace.py: python plan_refactor_compare.py PARENT THIS.
Kernel traces: name, grid, workgroup and LDS bytes of every launch, in order.  HIP traces: the API names, split into entries at
the script's hipDeviceSynchronize marks."""
import csv
import glob
import sys


def rows(d, suffix):
    files = sorted(glob.glob(f"{d}/**/*{suffix}", recursive=True))
    out = []
    for f in files:
        out += list(csv.DictReader(open(f)))
    return out


def kernels(d):
    r = sorted(rows(d, "kernel_trace.csv"), key=lambda x: int(x["Start_Timestamp"]))
    keys = ["Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size"]
    return [tuple(x[k] for k in keys) for x in r]


def api(d):
    r = sorted(rows(d, "hip_api_trace.csv"), key=lambda x: int(x["Start_Timestamp"]))
    names = [x["Function"] for x in r]
    parts, cur = [], []
    for n in names:
        if n == "hipDeviceSynchronize":
            parts.append(cur)
            cur = []
        else:
            cur.append(n)
    return parts + [cur]


a, b = sys.argv[1], sys.argv[2]
ka, kb = kernels(a), kernels(b)
if ka or kb:
    print(f"kernel launches: {len(ka)} / {len(kb)}; identical (name, grid, workgroup, LDS): {ka == kb}")
    for i, (x, y) in enumerate(zip(ka, kb)):
        if x != y:
            print("first difference at launch", i, x, y)
            break
pa, pb = api(a), api(b)
if any(pa) or any(pb):
    print(f"HIP API entries: {len(pa)} / {len(pb)}")
    for i, (x, y) in enumerate(zip(pa, pb)):
        same = x == y
        extra = ""
        if not same:
            import collections
            ca, cb = collections.Counter(x), collections.Counter(y)
            extra = f"  parent-only {dict(ca - cb)} this-only {dict(cb - ca)}"
        print(f"entry {i}: {len(x)} / {len(y)} calls, identical: {same}{extra}")
