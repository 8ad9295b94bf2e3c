"""Reference for the log-dir balance (kao_balance_logdirs), numpy + plain Python, no GPU: a restatement of the
synchronous rounds from the text of the definition, the lower bound, the brute-force move-stability check, the exhaustive optimum of
tiny brokers and the seeded instance families of the tests.  Loads stay below 2^62, so int64 holds them; keys are uint64; every
reported number is a Python int."""
import itertools

import numpy as np

from wleaders_ref import code

KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
SMALL_BASE = 4000
OPTIMUM_LIMIT = 70000   # placements the exhaustive optimum enumerates at most


def _arrays(dir_start, dir, size, base):
    ds = np.asarray(dir_start, dtype=np.int64).reshape(-1)
    d = np.asarray(dir, dtype=np.int64).reshape(-1)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    D = int(ds[-1])
    bs = np.zeros(D, dtype=np.int64) if base is None else np.asarray(base, dtype=np.int64).reshape(-1)
    assert ds[0] == 0 and (np.diff(ds) >= 0).all() and d.shape == w.shape and bs.shape == (D,) and (w >= 0).all() and (bs >= 0).all()
    assert not len(d) or (0 <= d.min() and d.max() < D)
    assert sum(int(x) for x in w) + sum(int(x) for x in bs) < 2 ** 62
    return ds, d, w, bs


def broker_of_dir(dir_start):
    ds = np.asarray(dir_start, dtype=np.int64)
    return np.repeat(np.arange(len(ds) - 1), np.diff(ds))


def loads(dir_start, dir, size, base=None):
    """L(d) = base[d] + the sizes of the replicas in d."""
    ds, d, w, bs = _arrays(dir_start, dir, size, base)
    out = bs.copy()
    np.add.at(out, d, w)
    return out


def ranking(L):
    """(order, rank): the dirs by load descending, ties by index ascending; rank 0 is the heaviest."""
    n = len(L)
    order = np.lexsort((np.arange(n), -L))
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    return order, rank


def _broker_rounds(L, a, w, ids, min_gain, max_rounds):
    """The rounds of ONE broker: L[n] its loads and a[k] the dirs of its replicas (indices inside the broker), both rewritten; w[k]
    the sizes, ids[k] the r of the keys.  Returns (rounds, moves, proposals, more)."""
    n, k = len(L), len(a)
    rounds = moves = proposals = 0
    more = False
    if n < 2 or k == 0 or min_gain >= 2 ** 62:   # no gap reaches 2^62
        return rounds, moves, proposals, more
    mg = np.int64(min_gain)
    wkey = ((np.uint64(0xFFFF) - code(w)) << np.uint64(32)) | ids.astype(np.uint64)
    pos = w > 0
    while True:
        order, rank = ranking(L)
        ra = rank[a]
        c1 = order[n - 1 - ra]
        c2 = np.full(k, order[n - 1], dtype=np.int64)
        ok1 = pos & (ra < n - 1 - ra) & (L[a] - L[c1] - w > mg)     # L(c1) + size + min_gain < L(a), without overflow
        ok2 = pos & ~ok1 & (ra >= 1) & (L[a] - L[c2] - w > mg)
        dest = np.where(ok1, c1, np.where(ok2, c2, -1))
        prop = dest >= 0
        if not prop.any():
            break
        if max_rounds > 0 and rounds >= max_rounds:
            more = True
            break
        rounds += 1
        proposals += int(prop.sum())
        key = (ra.astype(np.uint64) << np.uint64(48)) | wkey
        mk = np.full(n, KEY_NONE, dtype=np.uint64)
        np.minimum.at(mk, a[prop], key[prop])
        np.minimum.at(mk, dest[prop], key[prop])
        win = prop & (mk[a] == key) & (mk[np.maximum(dest, 0)] == key)
        assert win.any()                                    # the lowest key of all wins
        touched = np.concatenate([a[win], dest[win]])
        assert len(np.unique(touched)) == len(touched)      # winners share no dir
        peak, ssq = int(L.max()), sum(int(x) ** 2 for x in L)
        L[a[win]] -= w[win]
        L[dest[win]] += w[win]
        a[win] = dest[win]
        moves += int(win.sum())
        assert int(L.max()) <= peak and sum(int(x) ** 2 for x in L) < ssq
    return rounds, moves, proposals, more


def bound_terms(L0, w, bs):
    """The three terms of one broker's bound from its input loads, replica sizes and bases (n >= 1 dirs)."""
    n = len(L0)
    return [(max(int(x) for x in w) + min(int(x) for x in bs)) if len(w) else 0, -(-sum(int(x) for x in L0) // n), max(int(x) for x in bs)]


def descend(dir_start, dir, size, base=None, min_gain=0, max_rounds=0, ids=None):
    """The rounds of the definition, broker by broker.  ids[r] = the r of replica r's key (default: its index).  Returns a dict: dir,
    n_moved, bytes_moved, peak_before, peak_after, per_broker ([B][6] Python ints), status and stats (the eight of include/kao.h,
    stats[4] = None)."""
    ds, d, w, bs = _arrays(dir_start, dir, size, base)
    B = len(ds) - 1
    ids = np.arange(len(d), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    bod = broker_of_dir(ds)
    of = bod[d] if len(d) else np.zeros(0, dtype=np.int64)
    L_all = loads(ds, d, w, bs)
    out = d.copy()
    per, stats = [], [0] * 8
    stats[4] = None
    for b in range(B):
        lo, n = int(ds[b]), int(ds[b + 1] - ds[b])
        if n == 0:
            per.append([0] * 6)
            stats[6] += 1
            continue
        mine = np.nonzero(of == b)[0]
        L, a = L_all[lo:lo + n].copy(), d[mine] - lo
        terms = bound_terms(L, w[mine], bs[lo:lo + n])
        before = int(L.max())
        rounds, moves, props, more = _broker_rounds(L, a, w[mine], ids[mine], min_gain, max_rounds)
        out[mine] = a + lo
        ch = out[mine] != d[mine]
        per.append([before, int(L.max()), max(terms), int(ch.sum()), sum(int(x) for x in w[mine][ch]), rounds])
        stats[0] += rounds > 0
        stats[1] += rounds
        stats[2] += moves
        stats[3] += props
        stats[5] += int(more)
        stats[6] += int(L.max()) == max(terms)
        stats[7] = max(stats[7], rounds)
    assert int(loads(ds, out, w, bs).sum()) == int(L_all.sum())
    return dict(dir=out, n_moved=sum(p[3] for p in per), bytes_moved=sum(p[4] for p in per), peak_before=max((p[0] for p in per), default=0),
                peak_after=max((p[1] for p in per), default=0), per_broker=per, stats=stats,
                status="OPTIMAL_PROVEN" if stats[6] == B else "FEASIBLE_BOUND_GAP")


def lower_bound(dir_start, dir, size, base=None):
    """[B] the bound of every broker from the input alone (0 for a broker without dirs)."""
    ds, d, w, bs = _arrays(dir_start, dir, size, base)
    L = loads(ds, d, w, bs)
    of = broker_of_dir(ds)[d] if len(d) else np.zeros(0, dtype=np.int64)
    out = []
    for b in range(len(ds) - 1):
        lo, hi = int(ds[b]), int(ds[b + 1])
        out.append(max(bound_terms(L[lo:hi], w[of == b], bs[lo:hi])) if hi > lo else 0)
    return out


def stable(dir_start, dir, size, base=None, min_gain=0):
    """Brute force over every replica and every dir of its broker: no move r: a -> c with size > 0 has L(c) + size + min_gain < L(a)."""
    ds, d, w, bs = _arrays(dir_start, dir, size, base)
    if min_gain >= 2 ** 62 or not len(d):   # no gap reaches 2^62
        return True
    L = loads(ds, d, w, bs)
    of = broker_of_dir(ds)[d]
    for b in range(len(ds) - 1):
        lo, hi = int(ds[b]), int(ds[b + 1])
        mine = np.nonzero((of == b) & (w > 0))[0]
        if not len(mine) or hi - lo < 2:
            continue
        gap = L[d[mine]][:, None] - L[lo:hi][None, :] - w[mine][:, None]          # [replica, dir of the broker]
        other = np.arange(lo, hi)[None, :] != d[mine][:, None]
        if (other & (gap > np.int64(min_gain))).any():
            return False
    return True


def optimum(sizes, bases):
    """The lowest peak of any placement of the replicas `sizes` over one broker's dirs with `bases`, by enumeration; None when there
    are more than OPTIMUM_LIMIT placements."""
    n, w = len(bases), [int(x) for x in sizes]
    if n ** len(w) > OPTIMUM_LIMIT:
        return None
    best = None
    for place in itertools.product(range(n), repeat=len(w)):
        L = [int(x) for x in bases]
        for x, c in zip(w, place):
            L[c] += x
        best = max(L) if best is None else min(best, max(L))
    return best


def one_broker(case, b):
    """Broker b of a case as a case of its own, and the indices of its replicas in the case's arrays (the keys' r)."""
    ds, d, w, bs = _arrays(case["dir_start"], case["dir"], case["size"], case.get("base"))
    lo, hi = int(ds[b]), int(ds[b + 1])
    mine = np.nonzero((d >= lo) & (d < hi))[0]
    return dict(dir_start=np.array([0, hi - lo]), dir=d[mine] - lo, size=w[mine], base=bs[lo:hi]), mine


# ---- the seeded families ---------------------------------------------------------------------------------------------------------
def _skewed_dirs(rng, n, k):
    """k dirs out of n, dir i 1 / (i + 1) as likely as dir 0: the low dirs fill first."""
    p = 1.0 / (1.0 + np.arange(n))
    return rng.choice(n, size=k, p=p / p.sum()).astype(np.int64)


def small_case(seed):
    """dict(dir_start, dir, size, base): 1-6 brokers of 0-4 dirs, 0-8 replicas a broker with dirs, skewed toward its low dirs, a tenth
    of the sizes zero, a third of the dirs with a base; every tenth seed has all sizes equal.  The replicas of the brokers are
    interleaved in the arrays."""
    rng = np.random.default_rng(SMALL_BASE + seed)
    B = int(rng.integers(1, 7))
    nd = rng.integers(0, 5, B)
    dir_start = np.concatenate([[0], np.cumsum(nd)]).astype(np.int64)
    D = int(dir_start[-1])
    dirs = []
    for b in range(B):
        if nd[b]:
            dirs.append(dir_start[b] + _skewed_dirs(rng, int(nd[b]), int(rng.integers(0, 9))))
    d = np.concatenate(dirs).astype(np.int64) if dirs else np.zeros(0, dtype=np.int64)
    rng.shuffle(d)
    R = len(d)
    if seed % 10 == 0:
        size = np.full(R, 7, dtype=np.int64)
    elif seed % 3 == 2:
        size = np.round(np.exp(rng.normal(4.0, 1.0, R))).astype(np.int64)
    else:
        size = rng.integers(1, 50, R).astype(np.int64)
    size[rng.random(R) < 0.1] = 0
    base = np.where(rng.random(D) < 1 / 3, rng.integers(1, 80, D), 0).astype(np.int64)
    return dict(dir_start=dir_start, dir=d, size=size, base=base)


def crowded_case(n_dirs, n, base=0):
    """One broker, every replica on dir 0 of n_dirs: all proposals of a round have one source.  size = 5 everywhere when base == 0
    (every key ties down to r), else base + a small value."""
    size = np.full(n, 5, dtype=np.int64) if base == 0 else base + (np.arange(n) * 7919) % 13
    return dict(dir_start=np.array([0, n_dirs], dtype=np.int64), dir=np.zeros(n, dtype=np.int64), size=size.astype(np.int64), base=None)


def lognormal_case(n_brokers, n_dirs, n_replicas, sigma, seed, zeros=0.1, based=0.0):
    """n_brokers brokers of n_dirs dirs and n_replicas replicas each: a placement skewed 1:4 toward the high dirs, log-normal sizes
    around 2^20, a share `zeros` of them zero, a share `based` of the dirs with a base of a few replicas' bytes."""
    rng = np.random.default_rng(seed)
    p = 1.0 + 3.0 * np.arange(n_dirs) / max(n_dirs - 1, 1)
    local = rng.choice(n_dirs, size=(n_brokers, n_replicas), p=p / p.sum())
    d = (local + n_dirs * np.arange(n_brokers)[:, None]).reshape(-1).astype(np.int64)
    perm = rng.permutation(len(d))
    size = np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), sigma, len(d))))).astype(np.int64)
    size[rng.random(len(d)) < zeros] = 0
    D = n_brokers * n_dirs
    base = np.where(rng.random(D) < based, rng.integers(1, 8 << 20, D), 0).astype(np.int64)
    return dict(dir_start=(n_dirs * np.arange(n_brokers + 1)).astype(np.int64), dir=d[perm], size=size, base=base)
