"""Static tally of the dependent LDS round trips in k_search's iteration loop (hipcc -S -gline-tables-only), a sibling of loop_tally.py.
A trip is an `s_waitcnt` with an lgkmcnt field that guards a ds_read: at least one ds_read whose result has not been waited for is
outstanding, and the wait lets fewer operations stay in flight than have been issued since -- the wavefront stops there for an LDS
round trip.  Reads issued together and waited for once are one trip.  Per source region of kao_search.hip: ds_read / ds_write
instructions, trips, and the largest number of reads one trip waits for.  The regions are found by their comments, so the same script
walks the parent's and the branch's source; code of `finish` is charged to `finish@<the region that calls it>`, code of the headers to
the line of kao_search.hip it is inlined at.  A loop body counts once: in `fused scan` and `one-slot scan` the pair loop, the remainder
round and the weighted round are counted once each, whatever the number of rounds (the set-up and the rounds are one region: the
round's lambda stands in front of the loop that calls it).
Usage: trip_tally.py file.s kao_search.hip mangled-kernel-name-prefix"""
import re, sys, collections
src = open(sys.argv[1]).read().split("\n")
hip = open(sys.argv[2]).read().split("\n")
want = sys.argv[3]
def line_of(text, after=0):
    return next(i + 1 for i, l in enumerate(hip) if i >= after and text in l)
MARKS = [("loop head", "const uint32_t it = it_base + i;"), ("finish", "auto finish = [&]"), ("loop head", "constexpr std::integral_constant<int, 0> kReplace"),
         ("sampled REPLACE", "if (sampled) {"), ("LEADER-SWAP", "LEADER SWAP inside p"), ("tournament", "phase A: tournament"),
         ("second slot", "REPLACE scan (round 4)"), ("fused scan", "phase B (REPLACE), both tournament slots"),
         ("fused winner", "state after both slots' 2 n_rd draws"),
         ("one-slot scan", "the slot (p,k) of tournament lane wA"), ("EXCHANGE", "phase B (EXCHANGE)"), ("loop tail", "(one slot at a time)"),
         ("end of launch", "end of launch: verify the incremental bookkeeping")]
bounds, pos = [], 0
for name, text in MARKS:
    pos = line_of(text, pos)
    bounds.append((pos, name))
def region_of_line(n):
    r = None
    for first, name in bounds:
        if n >= first: r = name
    return r if r not in (None, "end of launch") else None
start = next(i for i, l in enumerate(src) if l.startswith(want) and ":" in l)
end = next(i for i in range(start + 1, len(src)) if src[i].strip().startswith(".amdhsa_kernel") or src[i].startswith("\t.section\t.rodata"))
tab = collections.defaultdict(collections.Counter)
region, pending, since = None, 0, 0   # pending: ds_reads not yet waited for; since: lgkm operations issued behind the oldest of them
for i in range(start, end):
    s = src[i].strip()
    if s.startswith(".loc"):
        frames = [int(n) for n in re.findall(r"kao_search\.hip:(\d+):", s)]
        if frames:
            r = region_of_line(frames[0])
            if r == "finish": r = "finish@" + (next((region_of_line(n) for n in frames[1:] if region_of_line(n) not in (None, "finish")), None) or "?")
            region = r
        continue
    if not s or s.startswith((";", ".")) or s.endswith(":"): continue
    op = s.split(";")[0].strip()
    o = op.split()[0]
    if o.startswith(("ds_read", "ds_bpermute", "ds_permute", "ds_swizzle")):
        if region: tab[region]["ds_read"] += 1
        pending += 1; since = since + 1 if pending > 1 else 1
    elif o.startswith(("ds_", "s_load", "s_buffer_load")):
        if region and o.startswith("ds_"): tab[region]["ds_write"] += 1
        if pending: since += 1
    elif o == "s_waitcnt":
        m = re.search(r"lgkmcnt\((\d+)\)", op)
        if m and pending and int(m.group(1)) < since:
            if region:
                tab[region]["trips"] += 1
                tab[region]["widest"] = max(tab[region]["widest"], pending)
            if int(m.group(1)) == 0: pending = since = 0
            else: since = int(m.group(1)); pending = min(pending, since)
print("%-28s %8s %8s %6s %7s" % ("region", "ds_read", "ds_write", "trips", "widest"))
tot = collections.Counter()
for r in sorted(tab, key=lambda r: (r.startswith("finish"), r)):
    c = tab[r]
    print("%-28s %8d %8d %6d %7d" % (r, c["ds_read"], c["ds_write"], c["trips"], c["widest"]))
    for k in ("ds_read", "ds_write", "trips"): tot[k] += c[k]
print("%-28s %8d %8d %6d" % ("ALL (static)", tot["ds_read"], tot["ds_write"], tot["trips"]))
