"""Reference logic for kao_plan_waves_headroom (tests only): the sequential loop of DESIGN.md section 4v run one priority order at
a time (the orders are those of waves_sized_ref.sized_order), the best-of rule, the order-count rule, an independent checker that
replays a wave[] on its own, and an exhaustive search over one-at-a-time orders for small instances.  Rows as in waves_ref."""
import numpy as np

from waves_ref import NONE, classify
from waves_sized_ref import lower_bound_sized, random_sized_instance, sized_order, traffic  # noqa: F401

UNLIMITED = 1 << 63
I64_MAX = (1 << 63) - 1


def add_rem(cur, tgt):
    """Per partition: (add = target \\ current in target order, rem = current \\ target in current order)."""
    out = []
    for c, n in zip(np.asarray(cur).tolist(), np.asarray(tgt).tolist()):
        cs, ns = {b for b in c if b != NONE}, {b for b in n if b != NONE}
        out.append(([b for b in n if b != NONE and b not in cs], [b for b in c if b != NONE and b not in ns]))
    return out


def stored_from_rows(cur, size, B):
    """stored[b] = the sum of size[p] over the current rows that hold b."""
    st = [0] * B
    for p, c in enumerate(np.asarray(cur).tolist()):
        for b in c:
            if b != NONE:
                st[b] += int(size[p])
    return st


def final_from_rows(tgt, size, B):
    return stored_from_rows(tgt, size, B)


def scaled_capacity(cur, tgt, size, B, s_num, s_den=100):
    """(stored, capacity) with capacity[b] = floor(max(stored[b], final[b]) * s_num / s_den), in integers."""
    st, fin = stored_from_rows(cur, size, B), final_from_rows(tgt, size, B)
    return st, [max(a, b) * s_num // s_den for a, b in zip(st, fin)]


def _fits(p, parts, traf, ar, size, occ, arr, cnt, byt, capacity, C, k):
    for b, t in zip(parts[p], traf[p]):
        if k and cnt.get(b, 0) >= k:
            return False
        l = byt.get(b, 0)
        if C and not (l == 0 or l + t <= C):
            return False
    sz = int(size[p])
    if sz:
        for b in ar[p][0]:
            if occ[b] + arr.get(b, 0) + sz > capacity[b]:
                return False
    return True


def run_order(cls, parts, traf, ar, size, stored, capacity, C, k, order):
    """One order: (wave per partition (moving ones: wave or -2), n_waves over moving partitions, (free, wave, broker) of the least
    free bytes over (wave, broker that receives bytes), or None)."""
    occ = [int(v) for v in stored]
    wave = {p: -2 for p in order}
    left = list(order)
    w, n_waves, least = 0, 0, None
    while True:
        cnt, byt, arr, dep = {}, {}, {}, {}
        if w == 0:
            for p, c in enumerate(cls):
                if c == 0:
                    for b in ar[p][1]:
                        dep[b] = dep.get(b, 0) + int(size[p])
        took, rest = False, []
        for p in left:
            if not _fits(p, parts, traf, ar, size, occ, arr, cnt, byt, capacity, C, k):
                rest.append(p)
                continue
            took = True
            wave[p] = w
            for b, t in zip(parts[p], traf[p]):
                cnt[b] = cnt.get(b, 0) + 1
                byt[b] = byt.get(b, 0) + t
            for b in ar[p][0]:
                arr[b] = arr.get(b, 0) + int(size[p])
            for b in ar[p][1]:
                dep[b] = dep.get(b, 0) + int(size[p])
        left = rest
        if not took and not any(dep.values()):
            break
        if took:
            n_waves = w + 1
        for b in sorted(arr):
            if arr[b] > 0:
                free = min(int(capacity[b]) - occ[b] - arr[b], I64_MAX)
                if least is None or free < least[0]:
                    least = (free, w, b)
        for b in set(arr) | set(dep):
            occ[b] += arr.get(b, 0) - dep.get(b, 0)
            assert occ[b] >= 0
        w += 1
    return wave, n_waves, least


def order_count(B, n_mv):
    """Orders one call runs: as many of the 64 as fit 1 GiB of per-order state, at least 1.  Per order: occ, arr, dep, byte loads
    (8 bytes each) and movement counts (4) per broker, three 8-byte minimum-key rows over the brokers, and per moving partition 4
    bytes of wave and 4 bytes of the wave it last skipped."""
    per_order = B * (4 * 8 + 4 + 3 * 8) + n_mv * 8
    return max(1, min(64, (1 << 30) // per_order))


def model(cur, tgt, size, stored, capacity, C, k, seed, n_orders=None):
    """What kao_plan_waves_headroom computes: (wave int64[P], n_waves, lower_bound, stats) with stats = [stuck, stuck bytes, winning
    order, orders run, None (launches: not modelled), least free, its wave, its broker]."""
    cls, parts, traf = traffic(cur, tgt, size)
    ar = add_rem(cur, tgt)
    B = len(stored)
    mv = [p for p, c in enumerate(cls) if c > 0]
    wave = np.array(cls, dtype=np.int64)
    base = 1 if any(c == 0 for c in cls) else 0
    lb = lower_bound_sized(cur, tgt, size, C, k)
    if not mv:
        return wave, base, lb, [0, 0, -1, 0, None, -1, -1, -1]
    n_ord = order_count(B, len(mv)) if n_orders is None else n_orders
    best = None
    for o in range(n_ord):
        wv, nw, least = run_order(cls, parts, traf, ar, size, stored, capacity, C, k, sized_order(parts, traf, o, seed))
        stuck = sum(1 for v in wv.values() if v == -2)
        nw = max(nw, base)
        if best is None or (stuck, nw) < best[:2]:
            best = (stuck, nw, o, wv, least)
    stuck, nw, o, wv, least = best
    for p in mv:
        wave[p] = wv[p]
    sb = min(sum(len(ar[p][0]) * int(size[p]) for p in mv if wv[p] == -2), I64_MAX)
    return wave, nw, lb, [stuck, sb, o, n_ord, None] + (list(least) if least else [-1, -1, -1])


def check_headroom(cur, tgt, size, stored, capacity, C, k, wave, n_waves, lb):
    """Replays wave[] on its own and asserts: the classes (-1 / 0 / wave or -2), both caps with the oversize rule,
    occ + arr <= capacity at every broker that receives bytes in every wave (departures free room only for later waves; the
    metadata-only partitions leave in wave 0), no wave below n_waves without a partition, the bound, and that every stuck
    partition fails the headroom test alone in the final state.  Returns the number of stuck partitions."""
    cls, parts, traf = traffic(cur, tgt, size)
    ar = add_rem(cur, tgt)
    wave = np.asarray(wave).tolist()
    assert len(wave) == len(cls)
    cnt, byt, pos = {}, {}, {}
    members = {}
    stuck = []
    for p, (c, w) in enumerate(zip(cls, wave)):
        if c < 0:
            assert w == -1, (p, w)
        elif c == 0:
            assert w == 0, (p, w)
            members.setdefault(0, []).append(p)
        elif w == -2:
            stuck.append(p)
        else:
            assert 0 <= w < n_waves, (p, w, n_waves)
            members.setdefault(w, []).append(p)
            for b, t in zip(parts[p], traf[p]):
                cnt[(w, b)] = cnt.get((w, b), 0) + 1
                byt[(w, b)] = byt.get((w, b), 0) + t
                pos[(w, b)] = pos.get((w, b), 0) + (t > 0)
    if k:
        assert all(v <= k for v in cnt.values()), max(cnt.values())
    if C:
        bad = [(key, v, pos[key]) for key, v in byt.items() if v > C and pos[key] != 1]
        assert not bad, bad[:5]
    assert set(members) == set(range(n_waves)), (sorted(members), n_waves)
    occ = [int(v) for v in stored]
    for w in range(n_waves):
        arr, dep = {}, {}
        for p in members[w]:
            for b in ar[p][0]:
                arr[b] = arr.get(b, 0) + int(size[p])
            for b in ar[p][1]:
                dep[b] = dep.get(b, 0) + int(size[p])
        for b, a in arr.items():
            assert a == 0 or occ[b] + a <= int(capacity[b]), (w, b, occ[b], a, int(capacity[b]))
        for b in set(arr) | set(dep):
            occ[b] += arr.get(b, 0) - dep.get(b, 0)
            assert occ[b] >= 0, (w, b)
    for p in stuck:
        sz = int(size[p])
        assert sz > 0 and any(occ[b] + sz > int(capacity[b]) for b in ar[p][0]), p
    ref = lower_bound_sized(cur, tgt, size, C, k)
    assert lb == ref, (lb, ref)
    if not stuck:
        assert n_waves >= lb
    return len(stuck)


def can_complete(cur, tgt, size, stored, capacity, max_moving=14):
    """Exhaustive: can some order that moves one partition at a time (each in a wave of its own, so its departure frees room
    for the next) complete the plan under the headroom rule alone?  The metadata-only partitions leave first.  None above
    `max_moving` moving partitions."""
    cls, _, _ = traffic(cur, tgt, size)
    ar = add_rem(cur, tgt)
    mv = [p for p, c in enumerate(cls) if c > 0]
    if len(mv) > max_moving:
        return None
    occ0 = [int(v) for v in stored]
    for p, c in enumerate(cls):
        if c == 0:
            for b in ar[p][1]:
                occ0[b] -= int(size[p])
    n = len(mv)
    delta = []
    for p in mv:
        d = {}
        for b in ar[p][0]:
            d[b] = d.get(b, 0) + int(size[p])
        for b in ar[p][1]:
            d[b] = d.get(b, 0) - int(size[p])
        delta.append(d)
    full = (1 << n) - 1
    seen = {0}
    stack = [0]
    while stack:
        m = stack.pop()
        if m == full:
            return True
        occ = list(occ0)
        for i in range(n):
            if m >> i & 1:
                for b, d in delta[i].items():
                    occ[b] += d
        for i in range(n):
            if m >> i & 1 or m | 1 << i in seen:
                continue
            p = mv[i]
            sz = int(size[p])
            if sz == 0 or all(occ[b] + sz <= int(capacity[b]) for b in ar[p][0]):
                seen.add(m | 1 << i)
                stack.append(m | 1 << i)
    return False
