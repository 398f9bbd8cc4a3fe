"""Per-dispatch SQ counters of k_schur from a rocprofv3 --pmc run (the output directory that
tools/pmc_sq.sh passes to rocprofv3 -d): one line per dispatch and template instance with its wave
count (grid / 64) and every counter's value, not the average over all matched dispatches.
usage: python tools/pmc_sq_dispatch.py <rocprofv3 output directory> [n_captures]"""
import collections
import csv
import glob
import sys

d = sys.argv[1]
nc = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rows = collections.OrderedDict()
for p in sorted(glob.glob(f"{d}/**/*counter_collection.csv", recursive=True)):
    for r in csv.DictReader(open(p)):
        k = r["Kernel_Name"]
        if "k_schur" not in k or "gather" in k or "combine" in k:
            continue
        key = (int(r["Dispatch_Id"]), k.replace("(anonymous namespace)::", "").split("(")[0])
        e = rows.setdefault(key, {"grid": int(r.get("Grid_Size", 0) or 0), "wg": int(r.get("Workgroup_Size", 0) or 0)})
        e[r["Counter_Name"]] = e.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
for (disp, name), e in rows.items():
    waves = e["grid"] // 64
    c = {k: int(v) for k, v in e.items() if k not in ("grid", "wg")}
    line = f"dispatch {disp} {name} grid {e['grid']} wg {e['wg']} waves {waves} {c}"
    if nc and "SQ_INSTS_VALU" in c:
        line += f"  VALU/capture wave {c['SQ_INSTS_VALU'] / nc:.1f}"
    print(line)
