"""Reference for the disk-usage balance by utilisation (kao_balance_disk_capacity), numpy + scipy, no GPU: the
rounds of tests/disk_ref.py and tests/disk_budget_ref.py with the four changes of the definition.  u(b) = S(b) / cap(b) is never a
quotient: x / cx is above y / cy iff x * cy > y * cx, products as Python ints (or int64 where the largest product is below 2^63).
  rank      by u descending, ties to the lower index;
  gain      (p, j, a -> c) passes iff (S(c) + size[p] + min_gain) * cap(a) < S(a) * cap(c), the sum below 2^64;
  rounds    FAST = the two walks of section 4m, each stopping at its first admissible, affordable broker, then the test; once a FAST
            round has no proposal every later round is THOROUGH: one walk over the ranks B-1 .. r+1 that proposes the first
            admissible, affordable broker that PASSES the test.  The descent ends when a THOROUGH round has no proposal;
  outputs   peaks and the bound are fractions {numerator, denominator}.
max_bytes = None is no budget."""
from fractions import Fraction

import numpy as np

import disk_budget_ref as br
import disk_ref as dr
from wleaders_ref import code

NONE = dr.NONE


def _ints(x):
    return [int(v) for v in np.asarray(x).reshape(-1)]


def ranking_cap(S, capv):
    """(order, rank): the brokers by S / cap descending, ties by index ascending; rank 0 is the fullest."""
    S, capv = _ints(S), _ints(capv)
    order = np.array(sorted(range(len(S)), key=lambda b: (-Fraction(S[b], capv[b]), b)), dtype=np.int64)
    rank = np.empty(len(S), dtype=np.int64)
    rank[order] = np.arange(len(S))
    return order, rank


def passes(S, capv, w, a, min_gain):
    """[P, B] bool: (S(c) + w[p] + min_gain) * cap(a[p]) < S(a[p]) * cap(c), the sum on the left below 2^64."""
    S, capv, w = (np.asarray(x, dtype=np.int64) for x in (S, capv, w))
    top = int(S.max(initial=0)) + int(w.max(initial=0)) + int(min_gain)
    if top * int(capv.max()) < 2 ** 63:
        return (S[None, :] + w[:, None] + np.int64(min_gain)) * capv[a][:, None] < (S[a] * 1)[:, None] * capv[None, :]
    So, co, wo = (np.array(_ints(x), dtype=object) for x in (S, capv, w))
    left = So[None, :] + wo[:, None] + int(min_gain)
    return ((left < 2 ** 64) & (left * co[a][:, None] < (So[a][:, None] * co[None, :]))).astype(bool)


def utilisations(S, capv):
    """The utilisations sorted descending, as Fractions."""
    return sorted((Fraction(s, c) for s, c in zip(_ints(S), _ints(capv))), reverse=True)


def peak_cap(S, capv):
    """(S(b*), cap(b*)) of the broker with the highest utilisation, ties to the lowest index."""
    S, capv = _ints(S), _ints(capv)
    b = min(range(len(S)), key=lambda i: (-Fraction(S[i], capv[i]), i))
    return S[b], capv[b]


def descend_cap(rows, size, B, rack_of, R, capacity, cap=0, move_leaders=True, min_gain=0, max_rounds=0, max_bytes=None):
    """The rounds of the definition.  Returns the dict of disk_budget_ref.descend with peak_before / peak_after as pairs, and:
    thorough (the THOROUGH rounds that had a proposal), utils (the sorted utilisation vector before the first round and after every
    round) and loads (the final S)."""
    rows = np.array(rows, dtype=np.int64)
    start = rows.copy()
    rk = np.asarray(rack_of, dtype=np.int64)
    capv = np.array(_ints(capacity), dtype=np.int64)
    P, W = rows.shape
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and rk.shape == (B,) and capv.shape == (B,)
    assert (capv >= 1).all() and sum(_ints(capv)) < 2 ** 62
    budget = 2 ** 64 - 1 if max_bytes is None else int(max_bytes)
    assert 0 <= budget < 2 ** 64 and 0 <= min_gain < 2 ** 64
    S = dr.loads(rows, w, B)
    assert int(S.sum()) < 2 ** 62
    S0 = S.copy()
    utils = [utilisations(S, capv)]
    rounds = moves = proposals = refused = spent = max_winners = thorough_rounds = 0
    top_rank = -1
    more = thorough = False
    first = 0 if move_leaders else 1
    if P:
        idx = np.arange(P)
        q = np.arange(B)[None, :]
        wcode = np.uint64(0xFFFF) - code(w)
        home = br.home_of(start, B)
        while True:
            rem = budget - spent
            fits = w <= min(rem, 2 ** 62)
            order, rank = ranking_cap(S, capv)
            held = rows != NONE
            safe = np.where(held, rows, 0)
            best_rank = np.full(P, B, dtype=np.int64)
            slot = np.zeros(P, dtype=np.int64)
            dest = np.full(P, -1, dtype=np.int64)
            for j in range(first, W):
                a = safe[:, j]
                r = rank[a][:, None]
                afford = home | (~home[idx, a])[:, None] | fits[:, None]
                ok_c = passes(S, capv, w, a, min_gain)                            # column = broker
                adm = (dr.admissible(rows, rk, R, cap, j) & afford)[:, order]     # column = rank
                c = np.full(P, -1, dtype=np.int64)
                if thorough:
                    qq = dr._first_from_top(adm & ok_c[:, order] & (q >= r + 1))
                    c = np.where(qq >= 0, order[np.maximum(qq, 0)], c)
                else:
                    q1 = dr._first_from_top(adm & (q >= r + 1) & (q <= B - 1 - r))
                    q2 = dr._first_from_top(adm & (q >= B - r))
                    for qq in (q2, q1):                                           # (the first walk's broker wins when both pass)
                        cc = order[np.maximum(qq, 0)]
                        c = np.where((qq >= 0) & ok_c[idx, cc], cc, c)
                ok = held[:, j] & (w > 0) & (c >= 0) & (rank[a] < best_rank)
                best_rank = np.where(ok, rank[a], best_rank)
                slot = np.where(ok, j, slot)
                dest = np.where(ok, c, dest)
            prop = dest >= 0
            if not prop.any():
                if thorough:
                    break
                thorough = True                                                   # an empty FAST round: every later round is THOROUGH
                continue
            if max_rounds > 0 and rounds >= max_rounds:
                more = True
                break
            rounds += 1
            thorough_rounds += int(thorough)
            proposals += int(prop.sum())
            a = rows[idx, slot]
            d = np.maximum(dest, 0)
            key = (best_rank.astype(np.uint64) << np.uint64(48)) | (wcode << np.uint64(32)) | idx.astype(np.uint64)
            mk = np.full(B, dr.KEY_NONE, dtype=np.uint64)
            np.minimum.at(mk, a[prop], key[prop])
            np.minimum.at(mk, dest[prop], key[prop])
            win = prop & (mk[a] == key) & (mk[d] == key)
            assert win.any()
            touched = np.concatenate([a[win], dest[win]])
            assert len(np.unique(touched)) == len(touched)                        # winners share no broker
            charge = np.where(win & ~home[idx, d] & home[idx, a], w, 0)
            wi = np.nonzero(win)[0]
            wi = wi[np.argsort(best_rank[wi], kind="stable")]
            assert len(np.unique(best_rank[wi])) == len(wi)
            cum = np.cumsum(charge[wi])
            ok = (charge[wi] == 0) | (cum <= min(rem, 2 ** 62))
            assert ok[0]                                                          # the lowest key of all is applied
            max_winners = max(max_winners, len(wi))
            top_rank = max(top_rank, int(best_rank[wi].max()))
            refused += int((~ok).sum())
            go = wi[ok]
            ua = {int(x): Fraction(int(S[x]), int(capv[x])) for x in a[go]}
            spent += sum(int(x) for x in ((~home[go, dest[go]]).astype(np.int64) - (~home[go, a[go]]).astype(np.int64)) * w[go])
            S[a[go]] -= w[go]
            S[dest[go]] += w[go]
            rows[go, slot[go]] = dest[go]
            for x, y in zip(a[go].tolist(), dest[go].tolist()):                   # a winner leaves both of its brokers strictly below the old u(a)
                assert Fraction(int(S[x]), int(capv[x])) < ua[x] and Fraction(int(S[y]), int(capv[y])) < ua[x]
            moves += len(go)
            assert spent == br.fresh_bytes(home, rows, w) <= budget
            utils.append(utilisations(S, capv))
    assert (S == dr.loads(rows, w, B)).all()
    n_moved, bytes_moved = dr.set_moves(start, rows, w)
    assert spent == bytes_moved
    bound = max_bytes is not None and not more and not stable_cap(rows, w, B, rk, R, capv, cap, move_leaders, min_gain)
    return dict(rows=rows, n_moved=n_moved, bytes_moved=bytes_moved, peak_before=peak_cap(S0, capv), peak_after=peak_cap(S, capv), rounds=rounds,
                moves=moves, proposals=proposals, more=more, rows_changed=int((rows != start).any(axis=1).sum()) if P else 0,
                brokers_changed=int((S != S0).sum()), refused=refused, spent=spent, budget_bound=bound, max_winners=max_winners, top_rank=top_rank,
                thorough=thorough_rounds, utils=utils, loads=S)


def stable_cap(rows, size, B, rack_of, R, capacity, cap=0, move_leaders=True, min_gain=0, start=None, rem=None):
    """Brute force over every movable slot and every broker: no admissible move (p, j, a -> c) with size > 0 passes the gain test.
    With `start` (the input rows) and `rem` only the moves whose charge is <= rem count."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    if not len(rows):
        return True
    S = dr.loads(rows, w, B)
    idx = np.arange(len(rows))
    home = None if start is None else br.home_of(start, B)
    for j in range(0 if move_leaders else 1, rows.shape[1]):
        held = (rows[:, j] != NONE) & (w > 0)
        a = np.where(held, rows[:, j], 0)
        ok = dr.admissible(rows, rack_of, R, cap, j) & passes(S, capacity, w, a, min_gain) & held[:, None]
        if home is not None:
            ok &= home | (~home[idx, a])[:, None] | (w <= min(int(rem), 2 ** 62))[:, None]
        if ok.any():
            return False
    return True


def lower_bound_cap(rows, size, B, capacity, move_leaders=True):
    """((numerator, denominator), term): the largest, as a fraction, of (0) {the largest size, the largest capacity}, (1) {the bytes
    stored, the sum of the capacities}, (2) with the leaders kept, {fixed(b), cap(b)} of the broker whose slot-0 bytes have the highest
    ratio (ties: the lowest index; {0, 1} when the leaders move); the lowest term on ties."""
    rows = np.asarray(rows, dtype=np.int64)
    w, capv = _ints(size), _ints(capacity)
    total = sum(int((r != NONE).sum()) * x for r, x in zip(rows, w))
    terms = [(max(w, default=0), max(capv)), (total, sum(capv)), (0, 1)]
    if not move_leaders:
        fixed = [0] * B
        for r, x in zip(rows.tolist(), w):
            fixed[r[0]] += x
        terms[2] = peak_cap(fixed, capv)
    best = max(range(3), key=lambda i: (Fraction(*terms[i]), -i))
    return terms[best], best


def integral_cap(peak, rows, size, capacity):
    """The integrality test: no placement puts every broker strictly below the utilisation peak = (S*, cap*): the sum over b of
    ceil(S* cap(b) / cap*) - 1 is below the bytes stored."""
    rows = np.asarray(rows, dtype=np.int64)
    total = sum(int((r != NONE).sum()) * x for r, x in zip(rows, _ints(size)))
    s, c = peak
    return sum(-(-s * x // c) - 1 for x in _ints(capacity)) < total


def proven_cap(peak, rows, size, B, capacity, move_leaders=True):
    """(proven, stats[6]): the peak equals the bound as fractions (the bound's term), or only the integrality test proves it (3)."""
    (n, d), term = lower_bound_cap(rows, size, B, capacity, move_leaders)
    if peak[0] * d == n * peak[1]:
        return True, term
    if integral_cap(peak, rows, size, capacity):
        return True, 3
    return False, term


def optimum_cap(rows, size, B, rack_of, R, capacity, cap=0, move_leaders=True, upper=None):
    """The lowest peak utilisation of any placement the moves could reach, as a Fraction, by HiGHS (scipy.optimize.milp) on the model
    of disk_ref.optimum.  A continuous "S(b) <= t cap(b), minimise t" takes HiGHS minutes on some of these instances, so the optimum
    is reached from above in INTEGER feasibility problems: given a placement of peak s / c (the input, or `upper`), is there one with
    S(b) <= ceil(s cap(b) / c) - 1 for every b, that is, with every broker strictly below s / c?  The answer's peak is recomputed in
    integers and asked about again; the first "infeasible" proves the optimum."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    rows = np.asarray(rows, dtype=np.int64)
    rk = np.asarray(rack_of, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    capv = _ints(capacity)
    P = len(rows)
    if P == 0:
        return Fraction(0)
    n = P * B
    k = (rows != NONE).sum(axis=1)
    cnt = dr.rack_counts(rows, rk, R)
    lb, ub = np.zeros(n), np.ones(n)
    A, lo, hi = [], [], []

    def row(entries, low, high):
        a = np.zeros(n)
        for i, v in entries:
            a[i] = v
        A.append(a)
        lo.append(low)
        hi.append(high)

    for p in range(P):
        row([(p * B + b, 1) for b in range(B)], k[p], k[p])
        if not move_leaders:
            lb[p * B + rows[p, 0]] = 1
        for r in range(R if cap > 0 else 0):
            row([(p * B + b, 1) for b in np.nonzero(rk == r)[0]], 0, max(cap, int(cnt[p, r])))
    first_load = len(A)
    for b in range(B):
        row([(p * B + b, float(w[p])) for p in range(P)], -np.inf, 0)
    A, lo, hi = np.array(A), np.array(lo, dtype=float), np.array(hi, dtype=float)
    best = peak_cap(dr.loads(rows, w, B), capv) if upper is None else tuple(upper)
    while best[0] > 0:
        limit = [-(-best[0] * c // best[1]) - 1 for c in capv]      # the largest S(b) strictly below best
        hi[first_load:] = limit
        res = milp(np.zeros(n), constraints=LinearConstraint(A, lo, hi), integrality=np.ones(n), bounds=Bounds(lb, ub))
        if res.status == 2:                                        # infeasible: no placement is strictly below best
            break
        assert res.status == 0, res.message
        x = np.round(res.x).reshape(P, B).astype(np.int64)
        assert (x.sum(axis=1) == k).all()
        S = (x * w[:, None]).sum(axis=0)
        assert all(int(s) <= l for s, l in zip(S, limit))
        best = peak_cap(S, capv)
    return Fraction(*best)


# ---- the seeded family -------------------------------------------------------------------------------------------------------------
def small_case_cap(seed):
    """disk_ref.small_case(seed) with capacities of four classes, 1000 .. 4000 plus a little."""
    c = dr.small_case(seed)
    rng = np.random.default_rng(9000 + seed)
    B = c["B"]
    c["capacity"] = (rng.choice([1, 2, 3, 4], B) * 1000 + rng.integers(0, 50, B)).astype(np.int64)
    return c
