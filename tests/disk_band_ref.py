"""Reference for the disk-usage balance inside a replica-count band (kao_balance_disk_banded), numpy + scipy,
no GPU: a restatement of the rounds from the text of the definition, which asserts the definition's own claims every round, the
brute-force stability check with both band tests, and the exact optimum inside the band by HiGHS.  What the definition calls
"unchanged" is taken from tests/disk_ref.py (loads, admissibility, rank, bound, families) and tests/disk_x_ref.py (the exchange
proposals of a round and exchange_stable).

THE DEFINITION, restated.  n(b) = the rows that contain b, partitions of size 0 included, taken like the loads as it stands at the
round's start.  A destination c must also have n(c) < hi; a slot on a is movable only if also n(a) > lo.  A MOVE round is a round of
kao_balance_disk under these two tests, and its winners also do n(a) -= 1, n(c) += 1.  With `exchange`, a round without a move
proposal is an EXCHANGE round of kao_balance_disk_exchange, untouched: it keeps every count."""
import numpy as np

import disk_ref as dr
import disk_x_ref as dx
from wleaders_ref import code

NONE = dr.NONE
KEY_NONE = dr.KEY_NONE
WIDE = (0, 2 ** 31 - 1)


def counts(rows, B):
    """n(b) = the number of rows that contain b."""
    rows = np.asarray(rows, dtype=np.int64)
    return np.bincount(rows[rows != NONE], minlength=B).astype(np.int64) if rows.size else np.zeros(B, dtype=np.int64)


def outside(n, band):
    """The brokers whose count is outside the band."""
    return int(((n < band[0]) | (n > band[1])).sum())


def _move_proposals(rows, w, S, n, order, rank, rk, R, band, cap, first, mg):
    """The move proposals of a round inside the band: (best_rank, slot, dest), dest -1 = none.  disk_ref.descend's round with
    ADMISSIBLE narrowed by n(c) < hi and MOVABLE by n(a) > lo."""
    P, W = rows.shape
    B = len(S)
    q = np.arange(B)[None, :]
    held = rows != NONE
    safe = np.where(held, rows, 0)
    room = (n < band[1])[order][None, :]                        # column = rank
    best_rank = np.full(P, B, dtype=np.int64)
    slot = np.zeros(P, dtype=np.int64)
    dest = np.full(P, -1, dtype=np.int64)
    for j in range(first, W):
        a = safe[:, j]
        r = rank[a][:, None]
        adm = dr.admissible(rows, rk, R, cap, j)[:, order] & room
        q1 = dr._first_from_top(adm & (q >= r + 1) & (q <= B - 1 - r))
        q2 = dr._first_from_top(adm & (q >= B - r))
        c = np.full(P, -1, dtype=np.int64)
        for qq in (q2, q1):                                     # (the first walk's broker wins when both pass)
            cc = order[np.maximum(qq, 0)]
            ok = (qq >= 0) & (S[a] - S[cc] - w > np.int64(mg))  # S(c) + w + min_gain < S(a), min_gain up to 2^62
            c = np.where(ok, cc, c)
        ok = held[:, j] & (w > 0) & (n[a] > band[0]) & (c >= 0) & (rank[a] < best_rank)
        best_rank = np.where(ok, rank[a], best_rank)
        slot = np.where(ok, j, slot)
        dest = np.where(ok, c, dest)
    return best_rank, slot, dest


def descend_band(rows, size, B, rack_of, R, band=WIDE, cap=0, move_leaders=True, min_gain=0, max_rounds=0, exchange=False):
    """The rounds of the definition.  Returns disk_x_ref.descend's dict (x_rounds, exchanges, x_proposals and x_peak are 0 without
    `exchange`) and: count_range (min, max of n before, then after), outside_before, outside_after, n0 and n (the counts)."""
    rows = np.array(rows, dtype=np.int64)
    start = rows.copy()
    rk = np.asarray(rack_of, dtype=np.int64)
    P, W = rows.shape
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    lo, hi = int(band[0]), int(band[1])
    assert w.shape == (P,) and (w >= 0).all() and rk.shape == (B,) and 0 <= lo <= hi
    S = dr.loads(rows, w, B)
    n = counts(rows, B)
    assert int(S.sum()) < 2 ** 62
    S0, n0 = S.copy(), n.copy()
    floor, ceil = np.minimum(lo, n0), np.maximum(hi, n0)        # what no count ever leaves
    t = dict(rounds=0, moves=0, proposals=0, more=False, x_rounds=0, exchanges=0, x_proposals=0, x_peak=0, kinds="")
    ssq = [sum(int(v) ** 2 for v in S)]
    peaks = [int(S.max(initial=0))]
    first = 0 if move_leaders else 1
    mg = min(int(min_gain), 2 ** 62)                            # every gap is below 2^62: nothing passes from there on
    seen_x = False
    if P:
        idx = np.arange(P)
        pi = [int(p) for p in np.lexsort((idx, -w)) if w[p] > 0]
        pos = {p: i for i, p in enumerate(pi)}
        wcode = np.uint64(0xFFFF) - code(w)
        while True:
            order, rank = dr.ranking(S)
            best_rank, slot, dest = _move_proposals(rows, w, S, n, order, rank, rk, R, (lo, hi), cap, first, mg)
            prop = dest >= 0
            xp = None
            if exchange and not prop.any():
                if not seen_x:
                    seen_x, t["x_peak"] = True, int(S.max())
                xp = dx._exchange_proposals(rows, w, S, order, rank, rk, R, cap, first, mg, pi, pos)
            if not prop.any() and not xp:
                break
            if max_rounds > 0 and t["rounds"] >= max_rounds:
                t["more"] = True
                break
            t["rounds"] += 1
            t["kinds"] += "m" if xp is None else "x"
            peak, before, excess = int(S.max()), ssq[-1], int((np.maximum(0, n - hi) + np.maximum(0, lo - n)).sum())
            if xp is None:                                      # ---- a MOVE round
                t["proposals"] += int(prop.sum())
                a = rows[idx, slot]
                assert (n[a[prop]] > lo).all() and (n[dest[prop]] < hi).all()
                key = (best_rank.astype(np.uint64) << np.uint64(48)) | (wcode << np.uint64(32)) | idx.astype(np.uint64)
                mk = np.full(B, KEY_NONE, dtype=np.uint64)
                np.minimum.at(mk, a[prop], key[prop])
                np.minimum.at(mk, dest[prop], key[prop])
                win = prop & (mk[a] == key) & (mk[np.maximum(dest, 0)] == key)
                assert win.any()                                # the lowest key of all wins
                touched = np.concatenate([a[win], dest[win]])
                assert len(np.unique(touched)) == len(touched)  # WINNERS SHARE NO BROKER: a count changes by at most one
                S[a[win]] -= w[win]
                S[dest[win]] += w[win]
                n[a[win]] -= 1
                n[dest[win]] += 1
                rows[idx[win], slot[win]] = dest[win]
                t["moves"] += int(win.sum())
            else:                                               # ---- an EXCHANGE round: section 4u's, untouched
                t["proposals"] += len(xp)
                t["x_proposals"] += len(xp)
                t["x_rounds"] += 1
                keys = {x: (q << 48) | ((0xFFFF - int(code(np.array([d], dtype=np.int64))[0])) << 32) | x for x, (j, y, k, a, c, d, q) in xp.items()}
                mk, pk = {}, {}
                for x, (j, y, k, a, c, d, q) in xp.items():
                    for word, at in ((mk, a), (mk, c), (pk, x), (pk, y)):
                        word[at] = min(word.get(at, keys[x]), keys[x])
                winners = [x for x, (j, y, k, a, c, d, q) in xp.items() if mk[a] == keys[x] and mk[c] == keys[x] and pk[x] == keys[x] and pk[y] == keys[x]]
                assert winners and min(keys, key=keys.get) in winners
                brokers = [b for x in winners for b in (xp[x][3], xp[x][4])]
                parts = [p for x in winners for p in (x, xp[x][1])]
                assert len(set(brokers)) == len(brokers) and len(set(parts)) == len(parts)
                for x in winners:
                    j, y, k, a, c, d, q = xp[x]
                    assert rows[x, j] == a and rows[y, k] == c and d > 0
                    S[a] -= d
                    S[c] += d
                    rows[x, j], rows[y, k] = c, a
                t["moves"] += len(winners)
                t["exchanges"] += len(winners)
            ssq.append(sum(int(v) ** 2 for v in S))
            peaks.append(int(S.max()))
            assert (S == dr.loads(rows, w, B)).all() and (n == counts(rows, B)).all()   # LOADS AND COUNTS AGREE WITH THE ROWS
            assert (n >= floor).all() and (n <= ceil).all()                             # NO COUNT LEAVES [min(lo, n0), max(hi, n0)]
            assert int((np.maximum(0, n - hi) + np.maximum(0, lo - n)).sum()) <= excess  # THE DISTANCE TO THE BAND NEVER RISES
            assert ssq[-1] < before and peaks[-1] <= peak                               # THE SUM OF SQUARES FALLS, THE PEAK NEVER RISES
            held = [[b for b in r if b != NONE] for r in rows.tolist()]
            assert all(len(set(r)) == len(r) for r in held)                             # NO BROKER TWICE IN A ROW
            assert dr.rack_rule_holds(start, rows, rk, R, cap)
            assert ((rows == NONE) == (start == NONE)).all() and (move_leaders or (rows[:, 0] == start[:, 0]).all())
    n_moved, bytes_moved = dr.set_moves(start, rows, w)
    t.update(rows=rows, n_moved=n_moved, bytes_moved=bytes_moved, peak_before=int(S0.max(initial=0)), peak_after=int(S.max(initial=0)),
             rows_changed=int((rows != start).any(axis=1).sum()) if P else 0, brokers_changed=int((S != S0).sum()), ssq=ssq, peaks=peaks,
             count_range=(int(n0.min()), int(n0.max()), int(n.min()), int(n.max())), outside_before=outside(n0, (lo, hi)), outside_after=outside(n, (lo, hi)),
             n0=n0, n=n)
    return t


def stable_band(rows, size, B, rack_of, R, band=WIDE, cap=0, move_leaders=True, min_gain=0):
    """Brute force over every movable slot and every broker, with both band tests: no admissible move (p, j, a -> c) with size > 0,
    n(a) > lo and n(c) < hi has S(c) + size + min_gain < S(a)."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    if not len(rows) or min_gain >= 2 ** 62:
        return True
    S = dr.loads(rows, w, B)
    n = counts(rows, B)
    for j in range(0 if move_leaders else 1, rows.shape[1]):
        held = (rows[:, j] != NONE) & (w > 0)
        a = np.where(held, rows[:, j], 0)
        held &= n[a] > band[0]
        gain = S[None, :] + w[:, None] + np.int64(min_gain) < S[a][:, None]
        if (dr.admissible(rows, rack_of, R, cap, j) & gain & held[:, None] & (n < band[1])[None, :]).any():
            return False
    return True


def optimum_band(rows, size, B, rack_of, R, band=WIDE, cap=0, move_leaders=True, upper=None):
    """The lowest peak of any placement inside the band: disk_ref.optimum's model plus one row per broker,
    min(lo, n0(b)) <= sum_p x[p, b] <= max(hi, n0(b)).  `upper` (the descent's own peak: its end state is a placement of the model)
    bounds the peak variable; an optimum above the model's lower bound is confirmed by a second solve that finds the model infeasible
    one below it, as disk_drain_ref.optimum_drain does.  The loads are integer variables of their own, S(b) = sum_p size[p] x[p, b], that sum
    to all the bytes, and HiGHS runs without its presolve: seed 42 of the small family (seven brokers, band 4..5, optimum one above
    the bound) takes 175 s with disk_ref.optimum's rows as they are."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    rows = np.asarray(rows, dtype=np.int64)
    rk = np.asarray(rack_of, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    P = len(rows)
    if P == 0:
        return 0
    n = P * B + B + 1                                      # x[p, b], then the loads S(b), then the peak
    k = (rows != NONE).sum(axis=1)
    cnt = dr.rack_counts(rows, rk, R)
    n0 = counts(rows, B)
    lb, ub = np.zeros(n), np.ones(n)
    lb[-1] = max(int(w.max()), -(-int((k * w).sum()) // B))
    ub[-1] = max(int(dr.loads(rows, w, B).max()) if upper is None else int(upper), lb[-1])
    ub[P * B:-1] = ub[-1]
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
    for b in range(B):
        row([(p * B + b, float(w[p])) for p in range(P)] + [(P * B + b, -1)], 0, 0)
        row([(P * B + b, 1), (n - 1, -1)], -np.inf, 0)
        row([(p * B + b, 1) for p in range(P)], min(int(band[0]), int(n0[b])), max(int(band[1]), int(n0[b])))
    row([(P * B + b, 1) for b in range(B)], int((k * w).sum()), int((k * w).sum()))
    c = np.zeros(n)
    c[-1] = 1
    con = LinearConstraint(np.array(A), np.array(lo, dtype=float), np.array(hi, dtype=float))

    def solve(top):
        """(status, peak recomputed in integers from the chosen placement) with the peak variable at most `top`."""
        hi_b = ub.copy()
        hi_b[-1] = top
        hi_b[P * B:-1] = np.minimum(hi_b[P * B:-1], top)
        res = milp(c, constraints=con, integrality=np.ones(n), bounds=Bounds(lb, hi_b), options={"mip_rel_gap": 0.9 / max(top, 1.0), "presolve": False})   # peaks are integers: a gap below 1 proves the optimum
        if res.status != 0:
            return res.status, None
        x = np.round(res.x[:P * B]).reshape(P, B).astype(np.int64)
        assert (x.sum(axis=1) == k).all()
        return 0, int((x * w[:, None]).sum(axis=0).max())

    status, opt = solve(ub[-1])
    assert status == 0, status
    while opt > lb[-1]:                                    # confirmed: nothing one below it (a placement found there is the new candidate)
        status, below = solve(opt - 1)
        if status != 0:
            assert status == 2, status                     # infeasible
            break
        assert below < opt
        opt = below
    return opt


# ---- the bands and the count-balanced family ---------------------------------------------------------------------------------------
def band_of(seed, n0):
    """The band of a seed, four in turn: wide open; (min n0, max n0), where the extremes are frozen; (floor(mean), ceil(mean)), where
    most brokers start outside; (floor(mean) - 1, ceil(mean) + 1)."""
    n0 = np.asarray(n0, dtype=np.int64)
    total, B = int(n0.sum()), len(n0)
    return (WIDE, (int(n0.min()), int(n0.max())), (total // B, -(-total // B)), (max(0, total // B - 1), -(-total // B) + 1))[seed % 4]


def balanced_case(B, P, W, sigma, seed, R=1):
    """dict as disk_ref.small_case (cap and move_leaders left to the caller): a COUNT-BALANCED start, row p on the brokers
    (p W + j) mod B of a seeded permutation of the brokers, the slots of a row shuffled, so that with B dividing P W every broker holds P W / B replicas; log-normal sizes
    around 2^20, none of them zero."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(B)
    rows = perm[(np.arange(P)[:, None] * W + np.arange(W)[None, :]) % B].astype(np.int64)
    for p in range(P):
        rows[p] = rng.permutation(rows[p])
    size = np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), sigma, P)))).astype(np.int64)
    return dict(rows=rows, size=size, B=B, rack_of=(np.arange(B) % R).astype(np.int64), R=R)


def run(c, band=WIDE, min_gain=0, max_rounds=0, exchange=False, **over):
    """descend_band on a case dict; `over` replaces cap / move_leaders."""
    c = dict(c, **over)
    return descend_band(c["rows"], c["size"], c["B"], c["rack_of"], c["R"], band, c.get("cap", 0), c.get("move_leaders", True), min_gain, max_rounds, exchange)
