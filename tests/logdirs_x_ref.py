"""Reference for the log-dir balance with exchange moves (kao_balance_logdirs_exchange), numpy + plain Python,
no GPU: a restatement of the two kinds of round from the text of the definition, which asserts the definition's own claims every
round, and the brute-force exchange-stability check.  The families, the loads, the ranking, the bound, `stable` and `optimum` are
those of tests/logdirs_ref.py.  Loads stay below 2^62, so int64 holds them; keys are uint64; every reported number is a Python int."""
import numpy as np

import logdirs_ref as lr
from wleaders_ref import code

KEY_NONE = lr.KEY_NONE
BRUTE_LIMIT = 96   # replicas of a broker up to which every exchange round checks COMPLETENESS against all pairs


def _move_proposals(L, a, w, pos, mg, order, rank):
    """The move proposals of kao_balance_logdirs: dest[k], -1 = none."""
    n, k = len(L), len(a)
    ra = rank[a]
    c1 = order[n - 1 - ra]
    c2 = np.full(k, order[n - 1], dtype=np.int64)
    ok1 = pos & (ra < n - 1 - ra) & (L[a] - L[c1] - w > mg)     # L(c1) + size + min_gain < L(a), without overflow
    ok2 = pos & ~ok1 & (ra >= 1) & (L[a] - L[c2] - w > mg)
    return np.where(ok1, c1, np.where(ok2, c2, -1))


def _passes(wx, wy, D, mg):
    """Candidate y passes for x: size[y] > 0, delta > 0, delta + min_gain < D (delta < D and D - delta > min_gain: no overflow)."""
    delta = wx - wy
    return (wy > 0) & (delta > 0) & (delta < D) & (D - delta > mg)


def _exchange_proposals(L, a, w, pos, mg, order, rank, pi, asc2):
    """The exchange proposals of one round: (dest[k], partner[k]), -1 = none.  pi = the replicas in the order PI (size descending,
    then r ascending), asc2 = 2 * the sizes ascending.  The walk goes rank by rank, lightest dir first, over all replicas at once."""
    n, k = len(L), len(a)
    dest, partner = np.full(k, -1, dtype=np.int64), np.full(k, -1, dtype=np.int64)
    ra = rank[a]
    place = np.empty(k, dtype=np.int64)   # the position of a replica in PI
    place[pi] = np.arange(k)
    for p in range(n - 1, 0, -1):
        c = int(order[p])
        on_c = np.sort(place[a == c])     # the positions of c's replicas in PI, ascending
        xs = np.nonzero(pos & (ra < p) & (dest < 0))[0]
        if not len(xs) or not len(on_c):
            continue
        D = L[a[xs]] - L[c]
        xs, D = xs[D > 0], D[D > 0]
        if not len(xs):
            continue
        g = k - np.searchsorted(asc2, 2 * w[xs] - D, side="right")   # replicas with 2 s > 2 size[x] - D
        i = np.searchsorted(on_c, g, side="left")
        has_lo, has_hi = i < len(on_c), i > 0
        y_lo = pi[on_c[np.minimum(i, len(on_c) - 1)]]
        y_hi = pi[on_c[np.maximum(i - 1, 0)]]
        ok_lo = has_lo & _passes(w[xs], w[y_lo], D, mg)
        ok_hi = has_hi & _passes(w[xs], w[y_hi], D, mg)
        far_lo, far_hi = np.abs(2 * (w[xs] - w[y_lo]) - D), np.abs(2 * (w[xs] - w[y_hi]) - D)
        take_hi = ok_hi & (~ok_lo | (far_hi < far_lo))               # a tie goes to y_lo
        y = np.where(take_hi, y_hi, y_lo)
        ok = ok_lo | ok_hi
        if k <= BRUTE_LIMIT:   # COMPLETENESS: if any y on c passes for x, one of the two candidates does
            every = np.nonzero(a == c)[0]
            brute = _passes(w[xs][:, None], w[every][None, :], D[:, None], mg).any(axis=1)
            assert (brute == ok).all()
        dest[xs[ok]] = c
        partner[xs[ok]] = y[ok]
    return dest, partner


def _broker_rounds(L, a, w, ids, min_gain, max_rounds, exchange=True):
    """The rounds of ONE broker: L[n] its loads and a[k] the dirs of its replicas (indices inside the broker), both rewritten; w[k]
    the sizes, ids[k] the r of the keys.  Returns a dict of counters: rounds, moves and proposals count both kinds."""
    n, k = len(L), len(a)
    t = dict(rounds=0, moves=0, proposals=0, more=False, x_rounds=0, exchanges=0, x_proposals=0, x_lowered=False)
    if n < 2 or k == 0 or min_gain >= 2 ** 62:   # no gap reaches 2^62
        return t
    mg = np.int64(min_gain)
    uid = ids.astype(np.uint64)
    wkey = ((np.uint64(0xFFFF) - code(w)) << np.uint64(32)) | uid
    pos = w > 0
    pi = np.lexsort((ids, -w))          # fixed for the whole call
    asc2 = np.sort(2 * w)
    first_exchange = True
    while True:
        order, rank = lr.ranking(L)
        ra = rank[a]
        dest = _move_proposals(L, a, w, pos, mg, order, rank)
        prop = dest >= 0
        is_x = exchange and not prop.any()
        if is_x:
            if first_exchange:   # IDENTITY: the state at the first exchange round is move-stable, the end state of kao_balance_logdirs
                assert not (pos & (L[a] - L.min() - w > mg)).any()
                first_exchange = False
            dest, partner = _exchange_proposals(L, a, w, pos, mg, order, rank, pi, asc2)
            prop = dest >= 0
        if not prop.any():
            break
        if max_rounds > 0 and t["rounds"] >= max_rounds:
            t["more"] = True
            break
        t["rounds"] += 1
        t["proposals"] += int(prop.sum())
        if is_x:
            delta = np.where(prop, w - w[np.maximum(partner, 0)], 0)
            key = (ra.astype(np.uint64) << np.uint64(48)) | ((np.uint64(0xFFFF) - code(delta)) << np.uint64(32)) | uid
        else:
            delta = w
            key = (ra.astype(np.uint64) << np.uint64(48)) | wkey
        assert len(np.unique(key[prop])) == int(prop.sum())   # keys are unique
        mk = np.full(n, KEY_NONE, dtype=np.uint64)
        np.minimum.at(mk, a[prop], key[prop])
        np.minimum.at(mk, dest[prop], key[prop])
        win = prop & (mk[a] == key) & (mk[np.maximum(dest, 0)] == key)
        assert win.any() and win[np.argmin(np.where(prop, key, KEY_NONE))]   # the lowest key of all wins
        touched = np.concatenate([a[win], dest[win]])
        assert len(np.unique(touched)) == len(touched)          # WINNERS ARE DISJOINT: they share no dir
        peak, ssq = int(L.max()), sum(int(x) ** 2 for x in L)
        src, dst, d_w = a[win].copy(), dest[win].copy(), delta[win].copy()
        if is_x:
            ys = partner[win]
            assert not win[ys].any() and len(np.unique(np.concatenate([np.nonzero(win)[0], ys]))) == 2 * len(ys)   # no replica touched twice
            assert (a[ys] == dst).all() and (d_w > 0).all() and (L[src] - L[dst] > d_w).all()
            drop = sum(2 * int(x) * (int(L[s]) - int(L[c]) - int(x)) for x, s, c in zip(d_w, src, dst))
            a[ys] = src
            t["x_rounds"] += 1
            t["exchanges"] += int(win.sum())
            t["x_proposals"] += int(prop.sum())
        old = L[src].copy()
        L[src] -= d_w
        L[dst] += d_w
        a[win] = dst
        t["moves"] += int(win.sum())
        after = sum(int(x) ** 2 for x in L)
        assert int(L.max()) <= peak and after < ssq             # THE PEAK NEVER RISES, the sum of squares falls
        assert (L[src] < old).all() and (L[dst] < old).all()    # both loads end strictly below the old L(a)
        if is_x:
            assert ssq - after == drop and drop > 0             # by 2 delta (D - delta) per exchange
            t["x_lowered"] |= int(L.max()) < peak
    return t


def descend(dir_start, dir, size, base=None, min_gain=0, max_rounds=0, ids=None, exchange=True):
    """The rounds of the definition, broker by broker.  ids[r] = the r of replica r's key (default: its index).  Returns a dict: dir,
    n_moved, bytes_moved, peak_before, peak_after, per_broker ([B][8] Python ints), status and stats (the twelve of include/kao.h,
    stats[4] = None).  exchange=False leaves the exchange rounds out: the numbers of logdirs_ref.descend in the shared places."""
    ds, d, w, bs = lr._arrays(dir_start, dir, size, base)
    B = len(ds) - 1
    ids = np.arange(len(d), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    bod = lr.broker_of_dir(ds)
    of = bod[d] if len(d) else np.zeros(0, dtype=np.int64)
    L_all = lr.loads(ds, d, w, bs)
    out = d.copy()
    per, stats = [], [0] * 12
    stats[4] = None
    for b in range(B):
        lo, n = int(ds[b]), int(ds[b + 1] - ds[b])
        if n == 0:
            per.append([0] * 8)
            stats[6] += 1
            continue
        mine = np.nonzero(of == b)[0]
        L, a = L_all[lo:lo + n].copy(), d[mine] - lo
        terms = lr.bound_terms(L, w[mine], bs[lo:lo + n])
        before = int(L.max())
        t = _broker_rounds(L, a, w[mine], ids[mine], min_gain, max_rounds, exchange)
        out[mine] = a + lo
        ch = out[mine] != d[mine]
        per.append([before, int(L.max()), max(terms), int(ch.sum()), sum(int(x) for x in w[mine][ch]), t["rounds"], t["x_rounds"], t["exchanges"]])
        stats[0] += t["rounds"] > 0
        stats[1] += t["rounds"]
        stats[2] += t["moves"]
        stats[3] += t["proposals"]
        stats[5] += int(t["more"])
        stats[6] += int(L.max()) == max(terms)
        stats[7] = max(stats[7], t["rounds"])
        stats[8] += t["x_rounds"]
        stats[9] += t["exchanges"]
        stats[10] += t["x_proposals"]
        stats[11] += int(t["x_lowered"])
    assert int(lr.loads(ds, out, w, bs).sum()) == int(L_all.sum())
    return dict(dir=out, n_moved=sum(p[3] for p in per), bytes_moved=sum(p[4] for p in per), peak_before=max((p[0] for p in per), default=0),
                peak_after=max((p[1] for p in per), default=0), per_broker=per, stats=stats,
                status="OPTIMAL_PROVEN" if stats[6] == B else "FEASIBLE_BOUND_GAP")


def exchange_stable(dir_start, dir, size, base=None, min_gain=0):
    """Brute force over every pair of replicas on two dirs of one broker: none has 0 < delta and delta + min_gain < D, with
    delta = size[x] - size[y] (size[y] > 0) and D = L(dir[x]) - L(dir[y])."""
    ds, d, w, bs = lr._arrays(dir_start, dir, size, base)
    if min_gain >= 2 ** 62 or not len(d):
        return True
    L = lr.loads(ds, d, w, bs)
    of = lr.broker_of_dir(ds)[d]
    for b in range(len(ds) - 1):
        mine = np.nonzero((of == b) & (w > 0))[0]
        if len(mine) < 2:
            continue
        delta = w[mine][:, None] - w[mine][None, :]
        D = L[d[mine]][:, None] - L[d[mine]][None, :]
        if ((delta > 0) & (delta < D) & (D - delta > np.int64(min_gain))).any():
            return False
    return True
