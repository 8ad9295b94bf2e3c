"""The resource table of the K-search family from `make resource-usage` remarks (hipcc -Rpass-analysis=kernel-resource-usage), set
against the `branch` rows of an earlier table: one `parent` and one `branch` line per kernel, and a last line that says whether any
kernel lost occupancy or gained scratch.
Usage: resource_table.py remarks.txt earlier_table.txt"""
import re, sys
rem = open(sys.argv[1]).read().split("\n")
old = {}
for l in open(sys.argv[2]):
    m = re.match(r"branch (\S+)\s+vgpr\s+(\d+) scratch\s+(\d+) waves/SIMD (\d+) sgpr_spill\s+(\d+) vgpr_spill\s+(\d+)", l)
    if m: old[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
def short(mangled):
    m = re.match(r"_ZN3kao(\d+)(k_\w+?)I(.*?)EEvNS_", mangled)
    if not m: return None
    name = m.group(2)[:int(m.group(1))]
    args = re.findall(r"L([bi])(\d+)E", m.group(3))
    return name + "<" + ",".join(v for _, v in args) + ">"
cur, rows = None, {}
for l in rem:
    m = re.search(r"remark: Function Name: (\S+)", l)
    if m: cur = short(m.group(1)); rows.setdefault(cur, {}) if cur else None; continue
    if cur is None: continue
    for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"),
                     ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)")):
        m = re.search(pat, l)
        if m: rows[cur][key] = int(m.group(1))
bad = []
fmt = "%-6s %-28s vgpr %3d scratch %3d waves/SIMD %d sgpr_spill %4d vgpr_spill %3d"
for name, r in rows.items():
    if not name or not name.startswith(("k_search", "k_team", "k_init")): continue
    new = (r["vgpr"], r["scratch"], r["waves"], r["sspill"], r["vspill"])
    if name in old:
        print(fmt % (("parent", name) + old[name]))
        if new[2] < old[name][2] or new[1] > old[name][1]: bad.append(name)
    print(fmt % (("branch", name) + new))
print("# lost occupancy or gained scratch:", " ".join(bad) or "none")
