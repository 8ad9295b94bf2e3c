"""Static VALU tally of k_search's iteration loop (hipcc -S -gline-tables-only), split by what the instruction is:
arithmetic, v_mov (VGPR->VGPR, SGPR->VGPR, constant), v_readlane that restores a spilled scalar, v_writelane that spills one, other lane
reads / writes -- per source region of kao_search.hip and in total.  The loop is every instruction from the first to the last one
whose .loc line lies between `const uint32_t it = it_base + i;` and the end-of-launch recount.  A spill register is a VGPR that
v_writelane fills from SGPRs at eight or more constant lanes.
Usage: loop_tally.py file.s kao_search.hip mangled-kernel-name-prefix [regions.txt]
regions.txt: lines `name first-line last-line` of kao_search.hip; the name `inherit` (a lambda several kinds inline, code of the
headers) charges an instruction to the region of the last instruction before it that has one."""
import re, sys, collections
src = open(sys.argv[1]).read().split("\n")
hip = open(sys.argv[2]).read().split("\n")
want = sys.argv[3]
regions = [l.split() for l in open(sys.argv[4]).read().split("\n") if l.strip()] if len(sys.argv) > 4 else []
loop_first = next(i + 1 for i, l in enumerate(hip) if "const uint32_t it = it_base + i;" in l)
loop_last = next(i + 1 for i, l in enumerate(hip) if "end of launch: verify the incremental bookkeeping" in l) - 1
start = next(i for i, l in enumerate(src) if l.startswith(want) and ":" in l)
end = next(i for i in range(start + 1, len(src)) if src[i].strip().startswith(".amdhsa_kernel") or src[i].startswith("\t.section\t.rodata"))
filenum = {}
for l in src:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m: filenum[int(m.group(1))] = (m.group(3) or m.group(2))
ins = []
cf, cl = 0, 0
for i in range(start, end):
    s = src[i].strip()
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
    if m: cf, cl = int(m.group(1)), int(m.group(2)); continue
    if not s or s.startswith(";") or s.startswith(".") or s.endswith(":"): continue
    ins.append((s.split(";")[0].strip(), cf, cl))
lanes = collections.defaultdict(set)
for op, _, _ in ins:
    m = re.match(r"v_writelane_b32 (v\d+), s\d+, (\d+)$", op)
    if m: lanes[m.group(1)].add(m.group(2))
SPILL = {v for v, ls in lanes.items() if len(ls) >= 8}
def own(cf): return "kao_search.hip" in filenum.get(cf, "")
def region(cf, cl):
    if not own(cf) or not cl: return "inherit"
    for name, a, b in regions:
        if int(a) <= cl <= int(b): return name
    return "other"
idx = [n for n, (_, cf, cl) in enumerate(ins) if own(cf) and loop_first <= cl <= loop_last]
tab = collections.defaultdict(collections.Counter)
last = "loop head"
for n in range(idx[0], idx[-1] + 1):
    op, cf, cl = ins[n]
    r = region(cf, cl)
    if r == "inherit": r = last
    else: last = r
    o = op.split()[0]
    a = [x.strip() for x in op.split(None, 1)[1].split(",")] if " " in op else []
    if not o.startswith("v_"):
        if o.startswith(("scratch_", "global_", "buffer_", "flat_")): tab[r]["vmem"] += 1; tab["ALL"]["vmem"] += 1
        elif o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop")): tab[r]["salu"] += 1; tab["ALL"]["salu"] += 1
        continue
    kind = "arith"
    if o.startswith("v_mov_b"):
        kind = "mov_vv" if a[1].startswith("v") else ("mov_sv" if re.match(r"(s\d|s\[|vcc|exec|ttmp)", a[1]) else "mov_c")
    elif o.startswith(("v_readlane", "v_readfirstlane")):
        kind = "rl_spill" if len(a) > 2 and a[1] in SPILL and a[2].isdigit() else "rl"
    elif o.startswith("v_writelane"):
        kind = "wl_spill" if a[0] in SPILL and a[1].startswith("s") and a[2].isdigit() else "wl"
    for k in (r, "ALL"):
        tab[k][kind] += 1; tab[k]["valu"] += 1
cols = ["valu", "arith", "mov_vv", "mov_sv", "mov_c", "rl_spill", "wl_spill", "rl", "wl", "vmem", "salu"]
print("spill VGPRs:", " ".join(sorted(SPILL)) or "-")
print("%-16s" % "region" + "".join("%9s" % c for c in cols))
for k in sorted(tab, key=lambda k: -tab[k]["valu"]):
    print("%-16s" % k + "".join("%9d" % tab[k][c] for c in cols))
