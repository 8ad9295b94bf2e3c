"""Reference for the disk-usage balance that empties brokers (kao_balance_disk_drain), numpy + scipy, no GPU: a
restatement of the rounds from the text of the definition, the lower bound over the live brokers, the brute-force checks (every
replica left on a draining broker is stranded; no move among the live brokers is left), the exact optimum by HiGHS with the draining
brokers closed, and the seeded family of draining sets.  tests/disk_ref.py is imported as it is."""
import numpy as np

import disk_ref as dr
from disk_ref import KEY_NONE, NONE
from wleaders_ref import code


def ranking_drain(S, drain):
    """(order, rank): draining brokers before every live one; inside each group load descending, then index ascending."""
    B = len(S)
    order = np.lexsort((np.arange(B), -S, np.asarray(drain) == 0))   # (the last key is the first criterion)
    rank = np.empty(B, dtype=np.int64)
    rank[order] = np.arange(B)
    return order, rank


def left_on(rows, size, drain):
    """(n_left, bytes_left): the replicas on draining brokers and their bytes."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    if not len(rows):
        return 0, 0
    on = (rows != NONE) & (np.asarray(drain)[np.where(rows != NONE, rows, 0)] != 0)
    return int(on.sum()), int((on.sum(axis=1) * w).sum())


def descend_drain(rows, size, B, rack_of, R, drain, cap=0, move_leaders=True, min_gain=0, max_rounds=0):
    """The rounds of the definition.  Returns disk_ref.descend's dict and n_left, bytes_left, drain_moves, last_drain_round (from 1; 0
    without a drain move) and replicas_left (the replicas on draining brokers before the first round and after every round)."""
    rows = np.array(rows, dtype=np.int64)
    start = rows.copy()
    rk = np.asarray(rack_of, dtype=np.int64)
    dn = np.asarray(drain).reshape(-1) != 0
    P, W = rows.shape
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and rk.shape == (B,) and dn.shape == (B,) and not dn.all()
    D = int(dn.sum())
    S = dr.loads(rows, w, B)
    assert int(S.sum()) < 2 ** 62
    S0 = S.copy()
    ssq = [sum(int(x) ** 2 for x in S)]
    peaks = [int(S.max())]
    left = [left_on(rows, w, dn)[0]]
    rounds = moves = proposals = drain_moves = last_drain_round = 0
    more = False
    first = 0 if move_leaders else 1
    mg = np.int64(min(int(min_gain), 2 ** 62))                 # no gap reaches 2^62: a larger min_gain tests the same
    if P:
        idx = np.arange(P)
        q = np.arange(B)[None, :]
        wcode = np.uint64(0xFFFF) - code(w)
        while True:
            order, rank = ranking_drain(S, dn)
            assert (dn[order[:D]]).all() and not dn[order[D:]].any()
            held = rows != NONE
            safe = np.where(held, rows, 0)
            best_rank = np.full(P, B, dtype=np.int64)          # the proposal of the slot whose broker ranks lowest
            slot = np.zeros(P, dtype=np.int64)
            dest = np.full(P, -1, dtype=np.int64)
            for j in range(W):
                a = safe[:, j]
                r = rank[a][:, None]
                leaves = held[:, j] & dn[a]                     # a slot on a draining broker: always movable, no gain test
                adm = dr.admissible(rows, rk, R, cap, j)[:, order] & (q >= D)   # column = rank; nothing moves onto a draining broker
                q1 = dr._first_from_top(adm & (q >= r + 1) & (q <= B - 1 - r))
                q2 = dr._first_from_top(adm & (q >= B - r))
                c = np.full(P, -1, dtype=np.int64)
                for qq in (q2, q1):                            # (the first walk's broker wins when both pass)
                    cc = order[np.maximum(qq, 0)]
                    ok = (qq >= 0) & (leaves | (S[a] - S[cc] - w > mg))
                    c = np.where(ok, cc, c)
                movable = leaves | (held[:, j] & (w > 0) & (j >= first))
                ok = movable & (c >= 0) & (rank[a] < best_rank)
                best_rank = np.where(ok, rank[a], best_rank)
                slot = np.where(ok, j, slot)
                dest = np.where(ok, c, dest)
            prop = dest >= 0
            if not prop.any():
                break
            if max_rounds > 0 and rounds >= max_rounds:
                more = True
                break
            rounds += 1
            proposals += int(prop.sum())
            a = rows[idx, slot]
            key = (best_rank.astype(np.uint64) << np.uint64(48)) | (wcode << np.uint64(32)) | idx.astype(np.uint64)
            mk = np.full(B, KEY_NONE, dtype=np.uint64)
            np.minimum.at(mk, a[prop], key[prop])
            np.minimum.at(mk, dest[prop], key[prop])
            win = prop & (mk[a] == key) & (mk[np.maximum(dest, 0)] == key)
            assert win.any()                                   # the lowest key of all wins
            touched = np.concatenate([a[win], dest[win]])
            assert len(np.unique(touched)) == len(touched)     # winners share no broker
            assert not dn[dest[win]].any()                     # nothing moves onto a draining broker
            S[a[win]] -= w[win]
            S[dest[win]] += w[win]
            rows[idx[win], slot[win]] = dest[win]
            moves += int(win.sum())
            gone = int((win & (best_rank < D)).sum())
            drain_moves += gone
            if gone:
                last_drain_round = rounds
            ssq.append(sum(int(x) ** 2 for x in S))
            peaks.append(int(S.max()))
            left.append(left_on(rows, w, dn)[0])
            assert left[-1] == left[-2] - gone and (gone or ssq[-1] < ssq[-2])   # why the rounds end
    assert (S == dr.loads(rows, w, B)).all()
    n_moved, bytes_moved = dr.set_moves(start, rows, w)
    n_left, bytes_left = left_on(rows, w, dn)
    return dict(rows=rows, n_moved=n_moved, bytes_moved=bytes_moved, peak_before=int(S0.max()), peak_after=int(S.max()), rounds=rounds, moves=moves,
                proposals=proposals, more=more, rows_changed=int((rows != start).any(axis=1).sum()) if P else 0,
                brokers_changed=int((S != S0).sum()), ssq=ssq, peaks=peaks, n_left=n_left, bytes_left=bytes_left, drain_moves=drain_moves,
                last_drain_round=last_drain_round, replicas_left=left)


def lower_bound_drain(rows, size, B, drain, move_leaders=True):
    """(bound, term) for every state with the draining brokers empty: the maximum of (0) the largest size, (1) the bytes shared among
    the live brokers, rounded up, (2) with the leaders kept, the largest sum of the slot-0 replicas that start on one live broker; term
    = the one that gives it, the lowest on ties."""
    rows = np.asarray(rows, dtype=np.int64)
    dn = np.asarray(drain).reshape(-1) != 0
    w = [int(x) for x in np.asarray(size).reshape(-1)]
    total = sum(int((r != NONE).sum()) * x for r, x in zip(rows, w))
    fixed = [0] * B
    if not move_leaders:
        for r, x in zip(rows.tolist(), w):
            if not dn[r[0]]:
                fixed[r[0]] += x
    terms = [max(w, default=0), -(-total // (B - int(dn.sum()))), max(fixed)]
    best = max(terms)
    return best, terms.index(best)


def stranded_reasons(rows, B, rack_of, R, drain, cap=0):
    """[(p, j, broker, reason)] of the replicas on draining brokers, reason = "row_holds_every_live_broker", "rack_rule", or None when a
    live broker is admissible (brute force over every live broker)."""
    rows = np.asarray(rows, dtype=np.int64)
    dn = np.asarray(drain).reshape(-1) != 0
    out = []
    if not len(rows):
        return out
    for j in range(rows.shape[1]):
        adm = dr.admissible(rows, rack_of, R, cap, j)
        free = dr.admissible(rows, rack_of, R, 0, j)           # not in the row
        for p in np.nonzero((rows[:, j] != NONE) & dn[np.where(rows[:, j] != NONE, rows[:, j], 0)])[0]:
            reason = None if adm[p, ~dn].any() else "rack_rule" if free[p, ~dn].any() else "row_holds_every_live_broker"
            out.append((int(p), j, int(rows[p, j]), reason))
    return sorted(out)


def left_is_stranded(rows, B, rack_of, R, drain, cap=0):
    """Every replica left on a draining broker has no admissible live broker."""
    return all(reason is not None for _, _, _, reason in stranded_reasons(rows, B, rack_of, R, drain, cap))


def stable_live(rows, size, B, rack_of, R, drain, cap=0, move_leaders=True, min_gain=0):
    """disk_ref.stable restricted to live sources and live destinations: no admissible move (p, j, a -> c) between two live brokers
    with size > 0 has S(c) + size + min_gain < S(a)."""
    rows = np.asarray(rows, dtype=np.int64)
    dn = np.asarray(drain).reshape(-1) != 0
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    if not len(rows) or min_gain >= 2 ** 62:
        return True
    S = dr.loads(rows, w, B)
    for j in range(0 if move_leaders else 1, rows.shape[1]):
        held = (rows[:, j] != NONE) & (w > 0)
        a = np.where(held, rows[:, j], 0)
        held &= ~dn[a]
        gain = S[None, :] + w[:, None] + np.int64(min_gain) < S[a][:, None]
        if (dr.admissible(rows, rack_of, R, cap, j) & gain & held[:, None] & ~dn[None, :]).any():
            return False
    return True


def optimum_drain(rows, size, B, rack_of, R, drain, cap=0, move_leaders=True, upper=None):
    """The lowest peak of any placement with the draining brokers empty: disk_ref.optimum's model with every x[p, b] of a draining b
    fixed to 0, slot 0 pinned only when it starts on a live broker, and the mean term over the live brokers.  `upper` is the peak of
    a placement of the model (the end of a descent that left nothing): it bounds the peak variable as the input's peak does in
    disk_ref.optimum, since the input itself is no placement here.  Without it the bound is all the bytes there are, and HiGHS then
    stops one above the optimum on seed 14 of the small family (910 for 909, reported as proven); so whatever the bound, an optimum
    above the model's lower bound is confirmed by a second solve that finds the model infeasible one below it.  Infeasible where a
    replica is stranded."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    rows = np.asarray(rows, dtype=np.int64)
    rk = np.asarray(rack_of, dtype=np.int64)
    dn = np.asarray(drain).reshape(-1) != 0
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    P = len(rows)
    if P == 0:
        return 0
    n = P * B + 1                                          # the last variable is the peak
    k = (rows != NONE).sum(axis=1)
    cnt = dr.rack_counts(rows, rk, R)
    lb, ub = np.zeros(n), np.ones(n)
    for b in np.nonzero(dn)[0]:
        ub[b:P * B:B] = 0
    lb[-1] = max(int(w.max()), -(-int((k * w).sum()) // (B - int(dn.sum()))))
    ub[-1] = max(int((k * w).sum()) if upper is None else int(upper), lb[-1])
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
        if not move_leaders and not dn[rows[p, 0]]:
            lb[p * B + rows[p, 0]] = 1
        for r in range(R if cap > 0 else 0):
            row([(p * B + b, 1) for b in np.nonzero(rk == r)[0]], 0, max(cap, int(cnt[p, r])))
    for b in range(B):
        row([(p * B + b, float(w[p])) for p in range(P)] + [(n - 1, -1)], -np.inf, 0)
    c = np.zeros(n)
    c[-1] = 1
    con = LinearConstraint(np.array(A), np.array(lo, dtype=float), np.array(hi, dtype=float))

    def solve(top):
        """(status, peak recomputed in integers from the chosen placement) with the peak variable at most `top`."""
        hi_b = ub.copy()
        hi_b[-1] = top
        res = milp(c, constraints=con, integrality=np.ones(n), bounds=Bounds(lb, hi_b), options={"mip_rel_gap": 0.9 / max(top, 1.0)})   # peaks are integers: a gap below 1 proves the optimum
        if res.status != 0:
            return res.status, None
        x = np.round(res.x[:-1]).reshape(P, B).astype(np.int64)
        assert (x.sum(axis=1) == k).all() and not x[:, dn].any()
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


def drain_of(seed, B):
    """[B] uint8: the draining set of a seed: one broker below 5 brokers, else one or two by the seed's parity."""
    rng = np.random.default_rng(7000 + seed)
    D = 1 if B < 5 else 1 + seed % 2
    out = np.zeros(B, dtype=np.uint8)
    out[rng.choice(B, D, replace=False)] = 1
    return out


def drain_flags(B, ids):
    out = np.zeros(B, dtype=np.uint8)
    out[list(ids)] = 1
    return out
