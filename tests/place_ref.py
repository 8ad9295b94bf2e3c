"""Reference for the log-dir placement (kao_place_logdirs), numpy + plain Python, no GPU: the sequential PLACE
from the text of the definition, the rounds of tests/logdirs_ref.py behind it, the generalised bound, the brute-force check that no
placed replica has an improving move, and the seeded family of the tests.  Every reported number is a Python int."""
import numpy as np

import logdirs_ref as lr

STAT_LAUNCHES = 5


def _arrays(dir_start, broker, dir, size, base):
    ds = np.asarray(dir_start, dtype=np.int64).reshape(-1)
    br = np.asarray(broker, dtype=np.int64).reshape(-1)
    d = np.asarray(dir, dtype=np.int64).reshape(-1)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    D, B = int(ds[-1]), len(ds) - 1
    bs = np.zeros(D, dtype=np.int64) if base is None else np.asarray(base, dtype=np.int64).reshape(-1)
    assert ds[0] == 0 and (np.diff(ds) >= 0).all() and br.shape == d.shape == w.shape and bs.shape == (D,) and (w >= 0).all() and (bs >= 0).all()
    if len(d):
        assert 0 <= br.min() and br.max() < B and d.min() >= -1
        res = d >= 0
        assert ((ds[br[res]] <= d[res]) & (d[res] < ds[br[res] + 1])).all()      # a resident sits in a dir of its broker
        assert (ds[br[~res] + 1] > ds[br[~res]]).all()                             # a homeless replica's broker has a dir
    assert sum(int(x) for x in w) + sum(int(x) for x in bs) < 2 ** 62
    return ds, br, d, w, bs


def order_of(w, ids):
    """The positions of `w` in the order size descending, then id ascending."""
    return np.lexsort((ids, -w))


def bound_terms(F, bs, w_res, w_home, move_residents):
    """The three terms of one broker's bound (n >= 1 dirs): F its loads before PLACE, bs its bases, the sizes of its residents and of
    its homeless replicas.  M = the homeless, or all with move_residents; F' = F, or base with move_residents."""
    n = len(F)
    m = [int(x) for x in w_home] + ([int(x) for x in w_res] if move_residents else [])
    fixed = [int(x) for x in (bs if move_residents else F)]
    return [(max(m) + min(fixed)) if m else 0, -(-(sum(fixed) + sum(m)) // n), max(fixed)]


def place(dir_start, broker, dir, size, base=None, move_residents=False, min_gain=0, max_rounds=0, ids=None):
    """kao_place_logdirs, broker by broker.  ids[r] = the r of replica r in the order of PLACE and in the keys of the rounds (default:
    its index).  Returns a dict: dir, n_placed, bytes_placed, n_moved, bytes_moved, peak_before, peak_after, per_broker ([B][8] Python
    ints), status and stats (the ten of include/kao.h, stats[5] = None)."""
    ds, br, d, w, bs = _arrays(dir_start, broker, dir, size, base)
    B = len(ds) - 1
    ids = np.arange(len(d), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    out = d.copy()
    per, stats = [], [0] * 10
    stats[STAT_LAUNCHES] = None
    for b in range(B):
        lo, n = int(ds[b]), int(ds[b + 1] - ds[b])
        if n == 0:
            per.append([0] * 8)
            stats[7] += 1
            continue
        mine = np.nonzero(br == b)[0]
        res, home = mine[d[mine] >= 0], mine[d[mine] < 0]
        F = bs[lo:lo + n].copy()
        np.add.at(F, d[res] - lo, w[res])
        terms = bound_terms(F, bs[lo:lo + n], w[res], w[home], move_residents)
        before = int(F.max())
        L = F.copy()
        for r in home[order_of(w[home], ids[home])]:     # PLACE: one replica after the other
            c = int(np.argmin(L))                        # the lowest load, ties to the lowest index
            L[c] += w[r]
            out[r] = lo + c
        rounds = moves = props = 0
        more = False
        if move_residents:
            a = out[mine] - lo
            rounds, moves, props, more = lr._broker_rounds(L, a, w[mine], ids[mine], min_gain, max_rounds)
            out[mine] = a + lo
        ch = out[res] != d[res]
        per.append([before, int(L.max()), max(terms), len(home), sum(int(x) for x in w[home]), int(ch.sum()), sum(int(x) for x in w[res][ch]), rounds])
        stats[0] += len(home) > 0
        stats[1] += rounds > 0
        stats[2] += rounds
        stats[3] += moves
        stats[4] += props
        stats[6] += int(more)
        stats[7] += int(L.max()) == max(terms)
        stats[8] = max(stats[8], rounds)
        stats[9] = max(stats[9], len(home))
    return dict(dir=out, n_placed=sum(p[3] for p in per), bytes_placed=sum(p[4] for p in per), n_moved=sum(p[5] for p in per),
                bytes_moved=sum(p[6] for p in per), peak_before=max((p[0] for p in per), default=0), peak_after=max((p[1] for p in per), default=0),
                per_broker=per, stats=stats, status="OPTIMAL_PROVEN" if stats[7] == B else "FEASIBLE_BOUND_GAP")


def lower_bound(dir_start, broker, dir, size, base=None, move_residents=False):
    """[B] the bound of every broker from the input alone (0 for a broker without dirs)."""
    ds, br, d, w, bs = _arrays(dir_start, broker, dir, size, base)
    out = []
    for b in range(len(ds) - 1):
        lo, hi = int(ds[b]), int(ds[b + 1])
        if hi == lo:
            out.append(0)
            continue
        res, home = np.nonzero((br == b) & (d >= 0))[0], np.nonzero((br == b) & (d < 0))[0]
        F = bs[lo:hi].copy()
        np.add.at(F, d[res] - lo, w[res])
        out.append(max(bound_terms(F, bs[lo:hi], w[res], w[home], move_residents)))
    return out


def placed_stable(dir_start, dir_in, dir_out, size, base=None):
    """Brute force over every placed replica (dir_in < 0) with size > 0 and every other dir of its broker: no move a -> c has
    L(c) + size < L(a) in the loads of dir_out."""
    ds = np.asarray(dir_start, dtype=np.int64)
    d0, d1, w = (np.asarray(x, dtype=np.int64) for x in (dir_in, dir_out, size))
    L = lr.loads(ds, d1, w, base)
    bod = lr.broker_of_dir(ds)
    for r in np.nonzero((d0 < 0) & (w > 0))[0]:
        a, b = int(d1[r]), int(bod[d1[r]])
        for c in range(int(ds[b]), int(ds[b + 1])):
            if c != a and int(L[c]) + int(w[r]) < int(L[a]):
                return False
    return True


def small_case(seed):
    """logdirs_ref.small_case(seed) with a broker array and about half of the replicas made homeless."""
    c = lr.small_case(seed)
    d = c["dir"].copy()
    broker = lr.broker_of_dir(c["dir_start"])[d] if len(d) else np.zeros(0, dtype=np.int64)
    d[np.random.default_rng(9000 + seed).random(len(d)) < 0.5] = -1
    return dict(dir_start=c["dir_start"], broker=broker.astype(np.int64), dir=d, size=c["size"], base=c["base"])


def one_broker(case, b):
    """Broker b of a case as a case of its own, and the indices of its replicas in the case's arrays (the r of the order and the keys)."""
    ds, br, d, w, bs = _arrays(case["dir_start"], case["broker"], case["dir"], case["size"], case.get("base"))
    lo, hi = int(ds[b]), int(ds[b + 1])
    mine = np.nonzero(br == b)[0]
    return dict(dir_start=np.array([0, hi - lo]), broker=np.zeros(len(mine), dtype=np.int64), dir=np.where(d[mine] >= 0, d[mine] - lo, -1), size=w[mine],
                base=bs[lo:hi]), mine
