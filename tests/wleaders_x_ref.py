"""Reference for the traffic-weighted leader balance with exchange moves (kao_balance_leaders_weighted_exchange, DESIGN.md section
4t), numpy + plain Python, no GPU: a restatement of the two kinds of round from the text of the definition, which asserts the
definition's own claims every round, and the brute-force exchange-stability check.  The families, the loads, the code, the bound,
`stable` and `optimum` are those of tests/wleaders_ref.py.  Loads stay below 2^62, so int64 holds them; keys are uint64; every
reported number is a Python int."""
import numpy as np

import wleaders_ref as wr

NONE = wr.NONE
KEY_NONE = wr.KEY_NONE
BRUTE_LIMIT = 100   # partitions up to which every exchange round checks COMPLETENESS against all pairs


def pair_index(rows, w):
    """(pi, segs): PI = the partitions by weight descending, then p ascending; segs[(lo, hi)] = the partitions with weight > 0 whose
    row holds both brokers, in the order PI.  Replica sets never change, so this is fixed for the call."""
    P = len(rows)
    pi = np.lexsort((np.arange(P), -w))
    segs = {}
    for p in pi.tolist():
        if w[p] <= 0:
            continue
        held = sorted(int(b) for b in rows[p] if b != NONE)
        for i in range(len(held)):
            for j in range(i + 1, len(held)):
                segs.setdefault((held[i], held[j]), []).append(p)
    return pi, {k: np.asarray(v, dtype=np.int64) for k, v in segs.items()}


def _passes(d, D, mg):
    """delta > 0 and delta + min_gain < D, in descent_gains' overflow-free form."""
    return (d > 0) & (d < D) & (D - d > mg)


def _brute_partner(x, a, c, rows, w, led, D, mg):
    """Does ANY y pass for (x, a <-> c)?  Every partition is tried: no index."""
    for y in range(len(rows)):
        if y == x or w[y] <= 0 or led[y] != c or a not in rows[y] or c not in rows[y]:
            continue
        d = int(w[x]) - int(w[y])
        if d > 0 and d < D and D - d > mg:
            return True
    return False


def _exchange_proposals(rows, w, lead, W, can, segs, mg):
    """The exchange proposals of one round: (slot[P], partner[P], delta[P]); slot -1 = none."""
    P = len(rows)
    slot, partner, delta = np.full(P, -1, dtype=np.int64), np.full(P, -1, dtype=np.int64), np.zeros(P, dtype=np.int64)
    led = rows[np.arange(P), lead]
    cache = {}
    Wl = W.tolist()
    for x in np.nonzero(can)[0].tolist():
        a, wx = int(led[x]), int(w[x])
        walk = sorted((Wl[b], j) for j, b in enumerate(rows[x].tolist()) if b != NONE and j != lead[x])   # W(c) ascending, ties: lowest slot
        first = None
        for Wc, j in walk:
            D = Wl[a] - Wc
            if D <= 0:
                continue
            c = int(rows[x, j])
            if (a, c) not in cache:   # S(a, c) without the test y != x: x is led by a, so it is never in it
                seg = segs.get((min(a, c), max(a, c)), np.zeros(0, dtype=np.int64))
                ys = seg[led[seg] == c]
                cache[(a, c)] = (ys, w[ys])
            ys, wy = cache[(a, c)]
            if P <= BRUTE_LIMIT and first is None and _brute_partner(x, a, c, rows, w, led, D, mg):
                first = j
            if not len(ys):
                continue
            d = wx - wy
            ok = _passes(d, D, mg)
            if not ok.any():
                continue
            i = np.nonzero(ok)[0]
            assert i[-1] - i[0] + 1 == len(i)              # the passing y are a contiguous run of S(a, c)
            run, heavy = ys[i], 2 * wy[i] > 2 * wx - D
            g = int(heavy.sum())
            assert heavy[:g].all()
            cand = []
            if g < len(run):
                cand.append((abs(2 * (wx - int(w[run[g]])) - D), 0, int(run[g])))        # y_lo; a tie goes to it
            if g > 0:
                cand.append((abs(2 * (wx - int(w[run[g - 1]])) - D), 1, int(run[g - 1])))  # y_hi
            y = min(cand)[2]
            slot[x], partner[x], delta[x] = j, y, wx - int(w[y])
            break
        if P <= BRUTE_LIMIT:   # COMPLETENESS: the first c with any passing y, among ALL partitions, is the proposal's
            assert (first if first is not None else -1) == slot[x], (x, first, slot[x])
    return slot, partner, delta


def descend(rows, weight, B, min_gain=0, max_rounds=0, exchange=True):
    """The rounds of the definition.  Returns wleaders_ref.descend's dict (rounds, moves and proposals count both kinds) and:
    x_rounds, exchanges, x_proposals, entries (of the pair index), first_x (the leader slots at the first exchange round; the end
    state when there is none), x_lowered (an exchange round lowered the peak)."""
    rows = np.asarray(rows, dtype=np.int64)
    P = len(rows)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and int(w.sum()) < 2 ** 62
    lead = np.zeros(P, dtype=np.int64)
    W = wr.loads(rows, w, B)
    before = int(W.max()) if B else 0
    t = dict(rounds=0, moves=0, proposals=0, more=False, x_rounds=0, exchanges=0, x_proposals=0, entries=0, first_x=None, x_lowered=False)
    if P:
        pi, segs = pair_index(rows, w)
        t["entries"] = sum(len(v) for v in segs.values())
    if P and min_gain < 2 ** 62:
        mg = int(min_gain)
        idx = np.arange(P)
        valid = rows != NONE
        safe = np.where(valid, rows, 0)
        can = (w > 0) & (valid.sum(axis=1) >= 2)
        big = np.int64(2 ** 63 - 1)
        while True:
            seen = np.where(valid, W[safe], big)
            seen[idx, lead] = big
            slot = np.argmin(seen, axis=1)            # the lowest load, ties to the lowest slot index
            a = rows[idx, lead]
            Wa, Wb = W[a], seen[idx, slot]
            prop = can & (Wb < big)
            prop &= (Wa - np.where(prop, Wb, 0) - w > np.int64(mg))       # W(b*) + w + min_gain < W(a)
            delta, partner = w, None
            is_x = exchange and not prop.any()
            if is_x:
                if t["first_x"] is None:
                    t["first_x"] = lead.copy()
                slot, partner, delta = _exchange_proposals(rows, w, lead, W, can, segs, mg)
                prop = slot >= 0
            if not prop.any():
                break
            if max_rounds > 0 and t["rounds"] >= max_rounds:
                t["more"] = True
                break
            t["rounds"] += 1
            t["proposals"] += int(prop.sum())
            b = safe[idx, np.maximum(slot, 0)]
            key = ((np.uint64(0xFFFF) - wr.code(Wa)) << np.uint64(48)) | ((np.uint64(0xFFFF) - wr.code(np.where(prop, delta, 0))) << np.uint64(32)) | idx.astype(np.uint64)
            mk = np.full(B, KEY_NONE, dtype=np.uint64)
            np.minimum.at(mk, a[prop], key[prop])
            np.minimum.at(mk, b[prop], key[prop])
            win = prop & (mk[a] == key) & (mk[b] == key)
            assert win.any() and win[np.argmin(np.where(prop, key, KEY_NONE))]   # the lowest key of all wins: every round applies something
            touched = np.concatenate([a[win], b[win]])
            assert len(np.unique(touched)) == len(touched)          # WINNERS ARE DISJOINT: they share no broker
            peak, ssq = int(W.max()), sum(int(v) ** 2 for v in W)
            src, dst, d_w = a[win].copy(), b[win].copy(), delta[win].copy()
            old = W[src].copy()
            if is_x:
                xs, ys = np.nonzero(win)[0], partner[win]
                assert len(np.unique(np.concatenate([xs, ys]))) == 2 * len(xs)      # no partition touched twice
                assert (rows[ys, lead[ys]] == dst).all() and (d_w > 0).all() and (old - W[dst] > d_w).all()
                drop = sum(2 * int(v) * (int(W[s]) - int(W[c]) - int(v)) for v, s, c in zip(d_w, src, dst))
                for x, y, s in zip(xs.tolist(), ys.tolist(), src.tolist()):
                    lead[y] = rows[y].tolist().index(s)            # j(y) = the slot of a in row y
                t["x_rounds"] += 1
                t["exchanges"] += len(xs)
                t["x_proposals"] += int(prop.sum())
            W[src] -= d_w
            W[dst] += d_w
            lead[win] = slot[win]
            t["moves"] += int(win.sum())
            after = sum(int(v) ** 2 for v in W)
            assert int(W.max()) <= peak and after < ssq             # THE PEAK NEVER RISES, the sum of squares falls
            assert (W[src] < old).all() and (W[dst] < old).all()    # both loads end strictly below the old W(a)
            if is_x:
                assert ssq - after == drop and drop > 0             # by 2 delta (D - delta) per exchange
                t["x_lowered"] |= int(W.max()) < peak
            assert (W == wr.loads(rows, w, B, lead)).all()
    if t["first_x"] is None:
        t["first_x"] = lead.copy()
    out = rows.copy()
    if P:
        out[np.arange(P), 0], out[np.arange(P), lead] = rows[np.arange(P), lead], rows[np.arange(P), 0]
    t.update(rows=out, lead=lead, n_changed=int((lead != 0).sum()), peak_before=before, peak_after=int(W.max()) if B else 0,
             leading=int(len(np.unique(out[:, 0]))) if P else 0)
    return t


def exchange_stable(rows_out, weight, B, min_gain=0):
    """Brute force over every pair of partitions (slot 0 leads): none has x led by a, y led by c, both rows holding both brokers,
    0 < delta and delta + min_gain < W(a) - W(c), with delta = weight[x] - weight[y] and weight[y] > 0."""
    rows = np.asarray(rows_out, dtype=np.int64)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    if min_gain >= 2 ** 62 or not len(rows):
        return True
    W = wr.loads(rows, w, B)
    held = np.zeros((len(rows), B), dtype=bool)
    for j in range(rows.shape[1]):
        ok = rows[:, j] != NONE
        held[np.nonzero(ok)[0], rows[ok, j]] = True
    a = rows[:, 0]
    both = held[:, a] & held[:, a].T                               # [x, y]: row x holds the leader of y and row y holds the leader of x
    d = w[:, None] - w[None, :]
    D = W[a][:, None] - W[a][None, :]
    bad = both & (w[None, :] > 0) & (d > 0) & (d < D) & (D - d > np.int64(min(int(min_gain), 2 ** 62)))
    return not bad.any()
