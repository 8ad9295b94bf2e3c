# Summarize rocprofv3 --pmc output of k_search (tools/profile_search_pmc.sh): mean counter value per dispatch, per kernel and grid size.
import sqlite3, glob, sys, os, csv
from collections import defaultdict
out = sys.argv[1]
g = defaultdict(lambda: defaultdict(list))
for db in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
    c = sqlite3.connect(db)
    try:
        rows = list(c.execute("select kernel_name, grid_size, workgroup_size, counter_name, value from counters_collection"))
    except Exception as e:
        print("db", db, e); continue
    for name, gs, wg, cn, val in rows:
        if "k_search" in name: g[(name[:60], gs // wg)][cn].append(val)
for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_search" in r.get("Kernel_Name", ""):
            g[(r["Kernel_Name"][:60], int(r["Grid_Size"]) // int(r["Workgroup_Size"]))][r["Counter_Name"]].append(float(r["Counter_Value"]))
for key, d in sorted(g.items()):
    print(key, {k: "%.4g" % (sum(v) / len(v)) for k, v in sorted(d.items())}, "n=%d" % min(len(v) for v in d.values()))
