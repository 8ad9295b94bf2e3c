"""Reference for the log-dir planners by utilisation (kao_balance_logdirs_capacity, kao_place_logdirs_capacity),
plain Python integers, no GPU: a restatement of the rounds, of PLACE, of the bound as a fraction and of the integrality test from the
text of the definition in include/kao.h, the brute-force move-stability check, the exhaustive optimum of tiny brokers and the seeded
family of the tests.  u(d) = L(d) / cap(d) is never a float or a quotient here either: fractions are compared by their products, and
Python's integers do not overflow.  Every reported number is a Python int."""
import itertools

import numpy as np

import logdirs_ref as lr
import place_ref as pr
from wleaders_ref import code_scalar

OPTIMUM_LIMIT = lr.OPTIMUM_LIMIT
KEY_NONE = 2 ** 64 - 1


def above(x, cx, y, cy):
    """x / cx > y / cy."""
    return x * cy > y * cx


def ranking(L, cap):
    """(order, rank): the dirs by L / cap descending, ties by index ascending; rank 0 is the fullest."""
    n = len(L)
    order = []
    for d in range(n):   # insertion: d goes before the first dir that is strictly emptier
        at = len(order)
        for i, e in enumerate(order):
            if above(L[d], cap[d], L[e], cap[e]):
                at = i
                break
        order.insert(at, d)
    rank = [0] * n
    for q, d in enumerate(order):
        rank[d] = q
    return order, rank


def gains(La, ca, Lc, cc, w, min_gain):
    """(L(c) + w + min_gain) * cap(a) < L(a) * cap(c); a left sum of 2^64 or more does not pass."""
    s = Lc + w + min_gain
    return s < 2 ** 64 and s * ca < La * cc


def proposal(L, cap, order, rank, a, w, min_gain):
    """(destination or None, how): how = "c1", "last" (the emptiest dir by the walk) or "walk" (a dir in between)."""
    n, q = len(L), rank[a]
    if w == 0 or n < 2:
        return None, None
    if q < n - 1 - q:
        c1 = order[n - 1 - q]
        if gains(L[a], cap[a], L[c1], cap[c1], w, min_gain):
            return c1, "c1"
    for p in range(n - 1, q, -1):
        c = order[p]
        if gains(L[a], cap[a], L[c], cap[c], w, min_gain):
            return c, "last" if p == n - 1 else "walk"
    return None, None


def sorted_utilisations(L, cap):
    order, _ = ranking(L, cap)
    return [(L[d], cap[d]) for d in order]


def _lex_below(x, y):
    """The utilisation lists x, y (sorted descending): x is lexicographically below y."""
    for (a, ca), (b, cb) in zip(x, y):
        if above(b, cb, a, ca):
            return True
        if above(a, ca, b, cb):
            return False
    return False


def broker_rounds(L, cap, a, w, ids, min_gain, max_rounds, trace=None):
    """The rounds of ONE broker: L[n] its loads and a[k] the dirs of its replicas (indices inside the broker), both rewritten; cap[n],
    w[k] the sizes, ids[k] the r of the keys.  Returns (rounds, moves, proposals, more).  trace (a dict) counts the proposals by kind
    and checks, round by round, that the peak utilisation does not rise and that the sorted utilisations fall."""
    n, k = len(L), len(a)
    rounds = moves = proposals = 0
    more = False
    while n >= 2 and k:
        order, rank = ranking(L, cap)
        props = []
        for i in range(k):
            c, how = proposal(L, cap, order, rank, a[i], w[i], min_gain)
            if c is not None:
                props.append((rank[a[i]] << 48 | (0xFFFF - code_scalar(w[i])) << 32 | ids[i], i, c))
                if trace is not None:
                    trace[how] = trace.get(how, 0) + 1
        if not props:
            break
        if max_rounds > 0 and rounds >= max_rounds:
            more = True
            break
        rounds += 1
        proposals += len(props)
        mk = [KEY_NONE] * n
        for key, i, c in props:
            mk[a[i]] = min(mk[a[i]], key)
            mk[c] = min(mk[c], key)
        wins = [(i, c) for key, i, c in props if mk[a[i]] == key and mk[c] == key]
        assert wins                                                        # the lowest key of all wins
        touched = [a[i] for i, _ in wins] + [c for _, c in wins]
        assert len(set(touched)) == len(touched)                           # winners share no dir
        before = sorted_utilisations(L, cap)
        for i, c in wins:
            old = (L[a[i]], cap[a[i]])
            L[a[i]] -= w[i]
            L[c] += w[i]
            assert above(*old, L[a[i]], cap[a[i]]) and above(*old, L[c], cap[c])   # both dirs strictly below the old u(a)
            a[i] = c
        moves += len(wins)
        after = sorted_utilisations(L, cap)
        assert not above(*after[0], *before[0]) and _lex_below(after, before)
    return rounds, moves, proposals, more


def frac_max(fr):
    """The largest fraction of a list of (num, den), the first on ties."""
    best = fr[0]
    for f in fr[1:]:
        if above(*f, *best):
            best = f
    return best


def frac_min(fr):
    best = fr[0]
    for f in fr[1:]:
        if above(*best, *f):
            best = f
    return best


def bound_terms(fixed, cap, m):
    """The three terms {num, den} of one broker's bound (n >= 1 dirs): fixed[d] = F'(d), m = the sizes of the replicas that may change
    dir.  Inside (0) and (2) ties go to the lowest dir."""
    t0 = frac_min([(f + max(m), c) for f, c in zip(fixed, cap)]) if m else (0, 1)
    return [t0, (sum(fixed) + sum(m), sum(cap)), frac_max(list(zip(fixed, cap)))]


def integrality(peak, fixed, cap, m):
    """room(d) = max(0, ceil(L* cap(d) / cap*) - 1 - F'(d)) cut at the bytes of M; passes iff the rooms sum to less than those bytes."""
    Ls, cs = peak
    total = sum(m)
    room = 0
    for f, c in zip(fixed, cap):
        room += min(total, max(0, -(-(Ls * c) // cs) - 1 - f))
    return room < total


def proof_of(peak, fixed, cap, m):
    """(bound {num, den}, proof): 1 = the peak equals the bound as fractions, 2 = the integrality test alone, 0 = a gap."""
    lb = frac_max(bound_terms(fixed, cap, m))
    if peak[0] * lb[1] == lb[0] * peak[1]:
        return lb, 1
    return lb, 2 if integrality(peak, fixed, cap, m) else 0


def _ints(x):
    return [int(v) for v in np.asarray(x).reshape(-1)]


def _call_peak(rows, nds, at):
    """{L, cap} of the fullest dir of the call from the rows of the brokers with dirs: ties to the lowest dir, {0, 1} without dirs."""
    fr = [(r[at], r[at + 1]) for r, n in zip(rows, nds) if n]
    return list(frac_max(fr)) if fr else [0, 1]


def descend(dir_start, dir, size, cap, base=None, min_gain=0, max_rounds=0, ids=None, trace=None):
    """kao_balance_logdirs_capacity, broker by broker.  Returns a dict: dir (int64 array), n_moved, bytes_moved, peak_before /
    peak_after ([L, cap]), per_broker ([B][10] Python ints), status, stats (the eight of include/kao.h, stats[4] = None)."""
    ds, d, w = _ints(dir_start), _ints(dir), _ints(size)
    B, D = len(ds) - 1, ds[-1]
    cp, bs = _ints(cap), ([0] * D if base is None else _ints(base))
    assert len(cp) == D and all(c >= 1 for c in cp) and sum(cp) < 2 ** 62 and sum(bs) + sum(w) < 2 ** 62
    ids = list(range(len(d))) if ids is None else _ints(ids)
    bod = _ints(lr.broker_of_dir(ds))
    out = list(d)
    per, stats = [], [0] * 8
    stats[4] = None
    for b in range(B):
        lo, n = ds[b], ds[b + 1] - ds[b]
        if n == 0:
            per.append([0, 1, 0, 1, 0, 1, 0, 0, 0, 1])
            stats[6] += 1
            continue
        mine = [r for r in range(len(d)) if bod[d[r]] == b]
        L, c = bs[lo:lo + n], cp[lo:lo + n]
        for r in mine:
            L[d[r] - lo] += w[r]
        before = frac_max(list(zip(L, c)))
        a = [d[r] - lo for r in mine]
        rounds, moves, props, more = broker_rounds(L, c, a, [w[r] for r in mine], [ids[r] for r in mine], min_gain, max_rounds, trace)
        for r, x in zip(mine, a):
            out[r] = lo + x
        after = frac_max(list(zip(L, c)))
        lb, proof = proof_of(after, bs[lo:lo + n], c, [w[r] for r in mine])
        ch = [r for r in mine if out[r] != d[r]]
        per.append([*before, *after, *lb, len(ch), sum(w[r] for r in ch), rounds, proof])
        stats[0] += rounds > 0
        stats[1] += rounds
        stats[2] += moves
        stats[3] += props
        stats[5] += int(more)
        stats[6] += proof > 0
        stats[7] = max(stats[7], rounds)
    nds = [ds[b + 1] - ds[b] for b in range(B)]
    return dict(dir=np.asarray(out, dtype=np.int64), n_moved=sum(p[6] for p in per), bytes_moved=sum(p[7] for p in per), peak_before=_call_peak(per, nds, 0),
                peak_after=_call_peak(per, nds, 2), per_broker=per, stats=stats, status="OPTIMAL_PROVEN" if stats[6] == B else "FEASIBLE_BOUND_GAP")


def place(dir_start, broker, dir, size, cap, base=None, move_residents=False, min_gain=0, max_rounds=0, ids=None, trace=None):
    """kao_place_logdirs_capacity, broker by broker.  Returns a dict: dir, n_placed, bytes_placed, n_moved, bytes_moved, peak_before /
    peak_after ([L, cap]), per_broker ([B][12] Python ints), status, stats (the ten of include/kao.h, stats[5] = None)."""
    ds, br, d, w = _ints(dir_start), _ints(broker), _ints(dir), _ints(size)
    B, D = len(ds) - 1, ds[-1]
    cp, bs = _ints(cap), ([0] * D if base is None else _ints(base))
    assert len(cp) == D and all(c >= 1 for c in cp) and sum(cp) < 2 ** 62 and sum(bs) + sum(w) < 2 ** 62
    ids = list(range(len(d))) if ids is None else _ints(ids)
    out = list(d)
    per, stats = [], [0] * 10
    stats[5] = None
    for b in range(B):
        lo, n = ds[b], ds[b + 1] - ds[b]
        mine = [r for r in range(len(d)) if br[r] == b]
        if n == 0:
            assert not mine
            per.append([0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1])
            stats[7] += 1
            continue
        res, home = [r for r in mine if d[r] >= 0], [r for r in mine if d[r] < 0]
        assert all(lo <= d[r] < lo + n for r in res)
        F, c = bs[lo:lo + n], cp[lo:lo + n]
        for r in res:
            F[d[r] - lo] += w[r]
        before = frac_max(list(zip(F, c)))
        L = list(F)
        for r in sorted(home, key=lambda r: (-w[r], ids[r])):      # PLACE: one replica after the other
            best = 0
            for x in range(1, n):                                   # the lowest (L + size) / cap, ties to the lowest index
                if above(L[best] + w[r], c[best], L[x] + w[r], c[x]):
                    best = x
            L[best] += w[r]
            out[r] = lo + best
        rounds = moves = props = 0
        more = False
        if move_residents:
            a = [out[r] - lo for r in mine]
            rounds, moves, props, more = broker_rounds(L, c, a, [w[r] for r in mine], [ids[r] for r in mine], min_gain, max_rounds, trace)
            for r, x in zip(mine, a):
                out[r] = lo + x
        after = frac_max(list(zip(L, c)))
        m = [w[r] for r in (mine if move_residents else home)]
        lb, proof = proof_of(after, bs[lo:lo + n] if move_residents else F, c, m)
        ch = [r for r in res if out[r] != d[r]]
        per.append([*before, *after, *lb, len(home), sum(w[r] for r in home), len(ch), sum(w[r] for r in ch), rounds, proof])
        stats[0] += len(home) > 0
        stats[1] += rounds > 0
        stats[2] += rounds
        stats[3] += moves
        stats[4] += props
        stats[6] += int(more)
        stats[7] += proof > 0
        stats[8] = max(stats[8], rounds)
        stats[9] = max(stats[9], len(home))
    nds = [ds[b + 1] - ds[b] for b in range(B)]
    return dict(dir=np.asarray(out, dtype=np.int64), n_placed=sum(p[6] for p in per), bytes_placed=sum(p[7] for p in per), n_moved=sum(p[8] for p in per),
                bytes_moved=sum(p[9] for p in per), peak_before=_call_peak(per, nds, 0), peak_after=_call_peak(per, nds, 2), per_broker=per, stats=stats,
                status="OPTIMAL_PROVEN" if stats[7] == B else "FEASIBLE_BOUND_GAP")


def loads(dir_start, dir, size, base=None):
    """L(d) as Python ints; replicas with dir < 0 are nowhere."""
    ds, d, w = _ints(dir_start), _ints(dir), _ints(size)
    L = [0] * ds[-1] if base is None else _ints(base)
    for r, x in enumerate(d):
        if x >= 0:
            L[x] += w[r]
    return L


def stable_cap(dir_start, dir, size, cap, base=None, min_gain=0, only=None):
    """Brute force over every replica (only: over those indices) with size > 0 and every other dir of its broker: no move r: a -> c
    passes the gain test in the loads of `dir`."""
    ds, d, w, cp = _ints(dir_start), _ints(dir), _ints(size), _ints(cap)
    L = loads(ds, d, w, base)
    bod = _ints(lr.broker_of_dir(ds))
    for r in (range(len(d)) if only is None else only):
        if w[r] == 0:
            continue
        a, b = d[r], bod[d[r]]
        for c in range(ds[b], ds[b + 1]):
            if c != a and gains(L[a], cp[a], L[c], cp[c], w[r], min_gain):
                return False
    return True


def optimum_cap(sizes, fixed, cap):
    """The lowest peak utilisation {L, cap} of any placement of the replicas `sizes` over one broker's dirs with the fixed loads
    `fixed`, by enumeration; None when there are more than OPTIMUM_LIMIT placements."""
    n, w = len(fixed), _ints(sizes)
    if n ** len(w) > OPTIMUM_LIMIT:
        return None
    best = None
    for where in itertools.product(range(n), repeat=len(w)):
        L = list(fixed)
        for x, c in zip(w, where):
            L[c] += x
        peak = frac_max(list(zip(L, cap)))
        if best is None or above(*best, *peak):
            best = peak
    return best


# ---- the seeded families ---------------------------------------------------------------------------------------------------------
def capacities(seed, n_dirs):
    """Seeded capacities: every tenth seed all equal, a third of the seeds from {100, 200, 400, 800}, the rest uniform in 20..399.
    The offset of the generator's seed is not arbitrary: brokers this small seldom end at an optimum that the integrality test alone
    proves (4 of 120 seeds is typical), so the offset was taken from a scan of 2,000 with this restatement as the one of three under
    which at least 10 seeds do, beside at least 10 with a proposal of the walk and 10 with a gap (tests/test_logdirs_cap_ref.py)."""
    rng = np.random.default_rng(222000 + seed)
    if seed % 10 == 0:
        return np.full(n_dirs, 300, dtype=np.int64)
    if seed % 3 == 2:
        return rng.choice(np.array([100, 200, 400, 800]), size=n_dirs).astype(np.int64)
    return rng.integers(20, 400, n_dirs).astype(np.int64)


def small_case_cap(seed):
    """logdirs_ref.small_case(seed) plus seeded capacities."""
    c = lr.small_case(seed)
    return dict(c, cap=capacities(seed, int(c["dir_start"][-1])))


def small_place_case_cap(seed):
    """place_ref.small_case(seed) plus the same capacities."""
    c = pr.small_case(seed)
    return dict(c, cap=capacities(seed, int(c["dir_start"][-1])))


def one_broker(case, b):
    """Broker b of a balance case as a case of its own, and the indices of its replicas (the keys' r)."""
    sub, mine = lr.one_broker(case, b)
    ds = _ints(case["dir_start"])
    return dict(sub, cap=np.asarray(case["cap"])[ds[b]:ds[b + 1]]), mine


def one_place_broker(case, b):
    sub, mine = pr.one_broker(case, b)
    ds = _ints(case["dir_start"])
    return dict(sub, cap=np.asarray(case["cap"])[ds[b]:ds[b + 1]]), mine
