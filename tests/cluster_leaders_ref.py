"""Test-side restatements of kao_balance_leaders_cluster: the preferred leaders of all topics chosen together,
replica sets kept, so that every topic's leader band holds, every broker leads at least LO partitions of the cluster, the largest
cluster-wide leader count is as low as it can be, and the fewest leaders change.

  lp            the HiGHS LP at a fixed cap M (a network matrix, so the LP value is the integer optimum); None = infeasible
  optimum       (peak, n_changed) by bisection over lp; None = infeasible at every cap
  enumerate_all the same by trying every choice (tiny instances)
  kernel_model  the kernels' probes and phases step by step (keys of (distance, arcs), lowest tight arc id as predecessor, deficit
                nodes served in index order, the sink's tight brokers in index order): rows, numbers and stats[0..4, 6, 7]
  launches      stats[5] from the solves kernel_model logged, as the entry point enqueues its kernels
and the instance families of the tests, those on the kernels' dispatch edges at the end.  Rows are [P, W] arrays of dense broker indices over one broker index, NONE-padded,
slot 0 = preferred leader; topic_of[p] is the topic of row p."""
import itertools

import numpy as np

NONE = 0xFFFF
INF = np.iinfo(np.int64).max
SOURCE = 1 << 62   # key of distance 0 and no arc: (distance + 2^30) << 32 | arcs


def _slots(rows):
    rows = np.asarray(rows, dtype=np.int64)
    P, W = rows.shape
    p = np.repeat(np.arange(P), W)
    j = np.tile(np.arange(W), P)
    keep = rows[p, j] != NONE
    return rows, p[keep], j[keep]


def lp(rows, topic_of, B, LO, M, tlo, thi):
    """min sum of x[p][j] over j != 0  s.t.  sum_j x[p][j] = 1;  tlo[t] <= L(t, b) <= thi[t] for every topic t and every broker b;
    LO <= L(b) <= M for every broker b.  None when infeasible."""
    from scipy import sparse
    from scipy.optimize import linprog
    rows, p, j = _slots(rows)
    topic_of = np.asarray(topic_of, dtype=np.int64)
    tlo, thi = np.asarray(tlo, dtype=np.int64), np.asarray(thi, dtype=np.int64)
    P, T, n = rows.shape[0], len(tlo), len(p)
    if P == 0:
        return 0 if LO == 0 and (tlo == 0).all() else None
    b = rows[p, j]
    t = topic_of[p]
    held = np.zeros((T, B), dtype=bool)
    held[t, b] = True
    if ((tlo > 0) & ~held.all(axis=1)).any():   # a broker that holds no replica of t leads none of it
        return None
    if M < LO or (LO > 0 and len(np.unique(b)) < B):
        return None
    var = np.arange(n)
    cost = (j != 0).astype(float)
    a_eq = sparse.csr_matrix((np.ones(n), (p, var)), shape=(P, n))
    pair, pair_idx = np.unique(t * B + b, return_inverse=True)
    per_pair = sparse.csr_matrix((np.ones(n), (pair_idx, var)), shape=(len(pair), n))
    per_broker = sparse.csr_matrix((np.ones(n), (b, var)), shape=(B, n))
    a_ub = sparse.vstack([per_pair, -per_pair, per_broker, -per_broker]).tocsr()
    b_ub = np.concatenate([thi[pair // B], -tlo[pair // B], np.full(B, M), np.full(B, -LO)]).astype(float)
    res = linprog(cost, A_ub=a_ub, b_ub=b_ub, A_eq=a_eq, b_eq=np.ones(P), bounds=(0, 1), method="highs")
    if res.status == 2:
        return None
    assert res.status == 0, res.message
    value = int(round(res.fun))
    assert abs(res.fun - value) < 1e-6, res.fun
    return value


def optimum(rows, topic_of, B, LO, tlo, thi):
    """None, or (the smallest cap M that is feasible, the fewest leader changes at that cap)."""
    P = len(rows)
    best = lp(rows, topic_of, B, LO, P, tlo, thi)
    if best is None:
        return None
    lo, hi = max(-(-P // B), LO), P
    while lo < hi:
        mid = (lo + hi) // 2
        v = lp(rows, topic_of, B, LO, mid, tlo, thi)
        if v is None:
            lo = mid + 1
        else:
            hi, best = mid, v
    return hi, best


def enumerate_all(rows, topic_of, B, LO, tlo, thi):
    """optimum() by trying every choice of leader slots."""
    rows = np.asarray(rows, dtype=np.int64)
    P = rows.shape[0]
    T = len(tlo)
    best = None
    for choice in itertools.product(*[[j for j in range(rows.shape[1]) if rows[p, j] != NONE] for p in range(P)]):
        L = np.zeros((T, B), dtype=np.int64)
        for p, j in enumerate(choice):
            L[topic_of[p], rows[p, j]] += 1
        tot = L.sum(axis=0)
        if (L < np.asarray(tlo)[:, None]).any() or (L > np.asarray(thi)[:, None]).any() or (tot < LO).any():
            continue
        cand = (int(tot.max()) if B else 0, sum(1 for j in choice if j))
        if best is None or cand < best:
            best = cand
    return best


def leader_counts(rows, topic_of, B, T):
    """L(t, b) of the rows' slot 0."""
    L = np.zeros((T, B), dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    if len(rows):
        np.add.at(L, (np.asarray(topic_of, dtype=np.int64), rows[:, 0]), 1)
    return L


def admissible(rows, topic_of, B, LO, M, tlo, thi):
    L = leader_counts(rows, topic_of, B, len(tlo))
    tot = L.sum(axis=0)
    return bool((L >= np.asarray(tlo)[:, None]).all() and (L <= np.asarray(thi)[:, None]).all() and (tot >= LO).all() and (tot <= M).all())


def check_rows(before, after):
    """Every output row is its input row with slot 0 and one non-empty slot swapped; returns the partitions changed."""
    before, after = np.asarray(before, dtype=np.int64), np.asarray(after, dtype=np.int64)
    assert before.shape == after.shape
    changed = 0
    for p in np.nonzero((before != after).any(axis=1))[0]:
        assert after[p, 0] != NONE, (p, before[p], after[p])
        j = int(np.nonzero(before[p] == after[p, 0])[0][0])
        want = before[p].copy()
        want[0], want[j] = want[j], want[0]
        assert j != 0 and (want == after[p]).all(), (p, before[p], after[p])
        changed += 1
    return changed


# ---- the kernels' schedule on the host -------------------------------------------------------------------------------------------
class _Net:
    def __init__(self, rows, topic_of, B, tlo, thi):
        self.rows = rows = np.asarray(rows, dtype=np.int64)
        self.P, self.W = rows.shape
        self.B = B
        topic_of = np.asarray(topic_of, dtype=np.int64)
        full = np.where(rows != NONE, topic_of[:, None] * B + rows, -1)
        keys = np.unique(full[full >= 0])
        self.Q = len(keys)
        self.pair_of = np.where(full >= 0, np.searchsorted(keys, full), -1)   # [P, W] dense pair index
        self.bro = keys % B
        self.top = keys // B
        self.plo = np.asarray(tlo, dtype=np.int64)[keys // B]
        self.phi = np.asarray(thi, dtype=np.int64)[keys // B]
        self.N = self.Q + B + 1
        self.T = self.Q + B
        self.c0 = np.bincount(self.pair_of[:, 0], minlength=self.Q).astype(np.int64) if self.P else np.zeros(self.Q, dtype=np.int64)
        self.claim = np.zeros(self.P, dtype=np.int64)
        self.stamp = 0
        self.stats = dict(probes=0, phases=0, rounds=0, paths=0, maxlen=0, left=0)
        self.solves = []   # per solve: dict(M, costed, rounds = the rounds of each phase, feasible, lead)


def _solve(net, LO, M, costed):
    """One solve at cap M from j = 0: (feasible, lead, f)."""
    rows, P, W, B, Q, N, T = net.rows, net.P, net.W, net.B, net.Q, net.N, net.T
    PW = P * W
    st = net.stats
    st["probes"] += 1
    lead = np.zeros(P, dtype=np.int64)
    g = np.clip(net.c0, net.plo, net.phi)
    inb = np.bincount(net.bro, weights=g, minlength=B).astype(np.int64)
    f = np.clip(inb, LO, M)
    e = np.concatenate([net.c0 - g, inb - f, [int(f.sum()) - P]])
    left = int(np.maximum(e, 0).sum())
    sp = np.repeat(np.arange(P), W)
    sj = np.tile(np.arange(W), P)
    ok_slot = net.pair_of[sp, sj] >= 0
    log = dict(M=M, costed=costed, rounds=[], feasible=False, lead=lead)
    net.solves.append(log)
    while left > 0:
        st["phases"] += 1
        log["rounds"].append(0)
        net.stamp += 1
        keep = ok_slot & (sj != lead[sp])
        ap, aj = sp[keep], sj[keep]
        au = net.pair_of[ap, lead[ap]]
        av = net.pair_of[ap, aj]
        ac = np.where(aj == 0, -1, np.where(lead[ap] == 0, 1, 0)) if costed else np.zeros(len(ap), dtype=np.int64)
        aid = ap * W + aj
        q = np.arange(Q)
        up, dn = q[g < net.phi], q[g > net.plo]
        bu, bd = np.nonzero(f < M)[0], np.nonzero(f > LO)[0]
        u = np.concatenate([au, up, Q + net.bro[dn], Q + bu, np.full(len(bd), T)])
        v = np.concatenate([av, Q + net.bro[up], dn, np.full(len(bu), T), Q + bd])
        c = np.concatenate([ac, np.zeros(len(up) + len(dn) + len(bu) + len(bd), dtype=np.int64)])
        ids = np.concatenate([aid, PW + up, PW + Q + dn, PW + 2 * Q + bu, PW + 2 * Q + B + bd])
        step = c * (1 << 32) + 1
        key = np.where(e > 0, SOURCE, INF).astype(np.int64)
        while True:
            st["rounds"] += 1
            log["rounds"][-1] += 1
            new = key.copy()
            ok = key[u] != INF
            np.minimum.at(new, v[ok], key[u[ok]] + step[ok])
            if (new == key).all():
                break
            key = new
        pred = np.full(N, 0xFFFFFFFF, dtype=np.int64)
        ok = key[u] != INF
        ok[ok] = key[u[ok]] + step[ok] == key[v[ok]]
        np.minimum.at(pred, v[ok], ids[ok])
        deficit = [int(t) for t in np.nonzero((e[:T] < 0) & (key[:T] != INF))[0]]
        targets = []
        if e[T] < 0 and key[T] != INF:
            kb = key[Q:Q + B]
            targets = [int(b) for b in np.nonzero((f < M) & (kb != INF) & ((kb >> 32) == (key[T] >> 32)))[0]]

        def walk(v0, apply):
            x, steps = v0, 0
            while key[x] & 0xFFFFFFFF:
                a = int(pred[x])
                steps += 1
                if a == 0xFFFFFFFF or steps > N:
                    return None
                if a < PW:
                    p = a // W
                    if not apply and net.claim[p] == net.stamp:
                        return None
                    y = int(net.pair_of[p, lead[p]])
                    if apply:
                        lead[p] = a - p * W
                        net.claim[p] = net.stamp
                elif a < PW + Q:
                    y = a - PW
                    if not apply and g[y] >= net.phi[y]:
                        return None
                    if apply:
                        g[y] += 1
                elif a < PW + 2 * Q:
                    qq = a - PW - Q
                    y = Q + int(net.bro[qq])
                    if not apply and g[qq] <= net.plo[qq]:
                        return None
                    if apply:
                        g[qq] -= 1
                elif a < PW + 2 * Q + B:
                    b = a - PW - 2 * Q
                    y = Q + b
                    if not apply and f[b] >= M:
                        return None
                    if apply:
                        f[b] += 1
                else:
                    b = a - PW - 2 * Q - B
                    y = T
                    if not apply and f[b] <= LO:
                        return None
                    if apply:
                        f[b] -= 1
                x = y
            return x

        naug = 0
        for t in deficit:
            while e[t] < 0:
                src = walk(t, False)
                if src is None or e[src] <= 0:
                    break
                walk(t, True)
                e[src] -= 1
                e[t] += 1
                naug += 1
                st["maxlen"] = max(st["maxlen"], int(key[t] & 0xFFFFFFFF))
        for b in targets:
            while e[T] < 0 and f[b] < M:
                src = walk(Q + b, False)
                if src is None or e[src] <= 0:
                    break
                walk(Q + b, True)
                f[b] += 1
                e[src] -= 1
                e[T] += 1
                naug += 1
                st["maxlen"] = max(st["maxlen"], int(key[Q + b] & 0xFFFFFFFF) + 1)
        st["paths"] += naug
        left -= naug
        if naug == 0:
            break
    st["left"] = left
    log["feasible"] = left == 0
    return left == 0, lead, f


def kernel_model(rows, topic_of, B, LO, tlo, thi, cluster_hi=-1, solves=None):
    """(feasible, output rows, n_changed, peak_before, peak_after, stats) as kao_balance_leaders_cluster reports them; stats[5], the
    launches, stays 0 (launches() states it).  A list given as `solves` takes one dict per solve in the order they run: its cap M,
    costed, the rounds of each of its phases (the quiet round included), feasible and the leader slots it ended with."""
    net = _Net(rows, topic_of, B, tlo, thi)
    if solves is not None:
        solves.clear()
        net.solves = solves
    rows = net.rows
    P = net.P
    peak_before = int(np.bincount(rows[:, 0], minlength=B).max()) if P else 0
    held = np.zeros((len(tlo), B), dtype=bool)
    held[net.top, net.bro] = True
    feasible = not ((np.asarray(tlo) > 0) & ~held.all(axis=1)).any()
    lead = np.zeros(P, dtype=np.int64)
    peak = peak_before
    if feasible:
        if cluster_hi >= 0:
            feasible, lead, f = _solve(net, LO, cluster_hi, True)
        else:
            feasible, lead, f = _solve(net, LO, max(P, LO), False)
            if feasible:
                lo, hi = max(-(-P // B), LO), int(f.max())
                while lo < hi:
                    mid = (lo + hi) // 2
                    ok, _, f = _solve(net, LO, mid, False)
                    if ok:
                        hi = int(f.max())
                    else:
                        lo = mid + 1
                feasible, lead, f = _solve(net, LO, hi, True)
                assert feasible
        if feasible:
            peak = int(f.max())
    s = net.stats
    stats = [s["probes"], s["phases"], s["rounds"], s["paths"], s["maxlen"], 0, net.Q, 0 if feasible else s["left"]]
    if not feasible:
        return False, rows.copy(), 0, peak_before, peak_before, stats
    out = rows.copy()
    idx = np.arange(P)
    out[idx, 0] = rows[idx, lead]
    out[idx, lead] = rows[idx, 0]
    return True, out, int((lead != 0).sum()), peak_before, peak, stats


def launches(P, solves, feasible):
    """stats[5] of kao_balance_leaders_cluster from the solves kernel_model logged, as the entry point enqueues them:
    the count (with any partition) and the input's peak; per solve the two start kernels and, when it is feasible, the peak of f; per
    phase the seed, the rounds in batches of eight between two reads of their flags (settle_rounds: a batch is enqueued whole), the
    predecessor bids and the extract; the apply of a feasible call with any partition."""
    n = (1 if P else 0) + 1
    for s in solves:
        n += 2 + sum(1 + 8 * -(-r // 8) + 2 for r in s["rounds"]) + (1 if s["feasible"] else 0)
    return n + (1 if feasible and P else 0)


# ---- instance families --------------------------------------------------------------------------------------------------------
def _row(rng, B, rf, hot, bias):
    r = rng.permutation(B)[:rf]
    if rng.random() < bias:                 # a hot broker leads when it holds a replica
        h = np.nonzero(r < hot)[0]
        if len(h):
            r[[0, h[0]]] = r[[h[0], 0]]
    return r


def small_case(seed):
    """rows [P, 3] (NONE-padded), topic_of, B, cluster_lo, tlo, thi"""
    rng = np.random.default_rng(seed)
    B = int(rng.integers(4, 13)); T = int(rng.integers(2, 6)); W = 3
    rows, topic_of, tlo, thi = [], [], [], []
    hot = int(rng.integers(1, max(2, B // 3) + 1))
    for t in range(T):
        Pt = int(rng.integers(3, 2 * B + 1)); rf = int(rng.integers(2, 4))
        for p in range(Pt):
            r = _row(rng, B, rf, hot, 0.6)
            rows.append(list(r) + [NONE] * (W - rf)); topic_of.append(t)
        s = int(rng.integers(0, 2)); tlo.append(max(0, Pt // B - s)); thi.append(-(-Pt // B) + s)
    LO = int(rng.integers(0, 2)) * (len(rows) // B // 2)
    return np.array(rows, dtype=np.int64), np.array(topic_of, dtype=np.int64), B, LO, np.array(tlo), np.array(thi)


def mid_case(B, T, Pt, rf, seed, hot_frac=0.1, pbias=0.5):
    """T topics of Pt partitions at RF rf on B brokers, the row recipe of small_case with hot = max(1, int(B * hot_frac)) and bias
    pbias, no padding: rows [T * Pt, rf], topic_of."""
    rng = np.random.default_rng(seed)
    hot = max(1, int(B * hot_frac))
    rows, topic_of = [], []
    for t in range(T):
        for p in range(Pt):
            rows.append(_row(rng, B, rf, hot, pbias)); topic_of.append(t)
    return np.array(rows, dtype=np.int64), np.array(topic_of, dtype=np.int64)


def tiny_case(seed):
    """At most 8 partitions, for enumeration: rows [P, 3], topic_of, B, cluster_lo, tlo, thi."""
    rng = np.random.default_rng(1000 + seed)
    B = int(rng.integers(2, 5)); T = int(rng.integers(1, 4)); W = 3
    rows, topic_of, tlo, thi = [], [], [], []
    left = 8
    for t in range(T):
        Pt = int(rng.integers(1, left - (T - 1 - t) + 1))   # every later topic keeps at least one partition
        left -= Pt
        rf = int(rng.integers(1, min(3, B) + 1))
        for p in range(Pt):
            r = _row(rng, B, rf, 1, 0.6)
            rows.append(list(r) + [NONE] * (W - rf)); topic_of.append(t)
        s = int(rng.integers(0, 2)); tlo.append(max(0, Pt // B - s)); thi.append(-(-Pt // B) + s)
    LO = int(rng.integers(0, 2))
    return np.array(rows, dtype=np.int64), np.array(topic_of, dtype=np.int64), B, LO, np.array(tlo), np.array(thi)


# ---- the dispatch edges of the kernels (tests/test_flow_paths_ref.py, tests/test_gpu_cluster_leaders_paths.py) -------------------
def chain(L, B=None):
    """Partitions [i, i + 1] for i < L and one more [0, 1], one topic with the band [0, P], cluster_lo = 0, cluster_hi = 1, B brokers
    (L + 1 when not given; the others idle): broker 0 leads two, and the one path runs from broker 0 to its pair, over the L partition
    arcs, to broker L and into the sink.  One solve of one phase, one path of L + 3 arcs, L + 4 rounds with the quiet one: (rows, topic_of, B, 0, [0], [P], 1)."""
    B = L + 1 if B is None else B
    assert L >= 1 and B >= L + 1
    rows = np.array([[i, i + 1] for i in range(L)] + [[0, 1]], dtype=np.int64)
    case = rows, np.zeros(L + 1, dtype=np.int64), B, 0, np.array([0]), np.array([L + 1]), 1
    solves = []
    ok, out, n, before, after, stats = kernel_model(*case, solves=solves)
    assert ok and (n, before, after) == (L, 2, 1) and (out[:L] == rows[:L, ::-1]).all() and (out[L] == rows[L]).all()
    assert [s["rounds"] for s in solves] == [[L + 4]] and stats[:5] == [1, 1, L + 4, 1, L + 3]
    return case


def probes_case():
    """P = 257 partitions of one topic on four brokers (Q = 4), cluster_hi = -1.  Broker 0 leads 104, and only the last three rows
    (254, 255, 256) can move, one to each other broker; row 256 is the only way into broker 3.  The bisection runs infeasible probes
    that move all three, then feasible ones: a solve that did not start from lead[256] = 0 (the row sits in the second block of
    256) finds no arc into broker 3 and calls the optimum, 101, infeasible."""
    one = lambda b, n: [[b, NONE, NONE]] * n
    rows = np.array(one(0, 101) + one(1, 60) + one(2, 60) + one(3, 33) + [[0, 1, NONE], [0, 2, NONE], [0, 3, NONE]], dtype=np.int64)
    case = rows, np.zeros(len(rows), dtype=np.int64), 4, 0, np.array([0]), np.array([len(rows)])
    solves = []
    ok, out, n, before, after, stats = kernel_model(*case, solves=solves)
    assert len(rows) == 257 and stats[6] == 4 and ok and (n, before, after) == (3, 104, 101) and stats[0] >= 4
    moved = [int(s["lead"][256]) for s in solves]
    assert moved[-1] == 1 and any(m == 1 and not s["feasible"] for m, s in zip(moved[:-1], solves)), moved
    return case


def wide_index_case():
    """chain(5) among 600 brokers: N = Q + B + 1 = 607 nodes against PW = 12 slots, so the grid of the rounds comes from N."""
    case = chain(5, 600)
    assert _Net(case[0], case[1], 600, case[4], case[5]).N > case[0].size
    return case


def deficit_case(extra):
    """cluster_lo = 1 on 32 brokers: rows [k, 16 + k] twice for k < 16, so brokers 16..31 lead nothing and are deficit nodes.  With
    extra = 0 one topic: Q = 32, T = 64, the last deficit node is 63 = T - 1, the last of the one 64-wide ballot.  With extra = 1 a
    second topic of one row [0] adds a pair: Q = 33, T = 65, deficit nodes at 63 and at 64 = T - 1, alone in the second ballot."""
    rows = [[p // 2, 16 + p // 2] for p in range(32)] + [[0, NONE]] * extra
    topic_of = [0] * 32 + [1] * extra
    case = np.array(rows, dtype=np.int64), np.array(topic_of, dtype=np.int64), 32, 1, np.zeros(1 + extra, dtype=np.int64), np.full(1 + extra, 2)
    net = _Net(case[0], case[1], 32, case[4], case[5])
    inb = np.bincount(net.bro, weights=np.clip(net.c0, net.plo, net.phi), minlength=32)
    nodes = (net.Q + np.nonzero(inb < 1)[0]).tolist()
    assert net.T == 64 + extra and net.T % 64 == extra and 63 in nodes and net.T - 1 in nodes and (extra == 0 or 64 in nodes), nodes
    ok, _, n, before, after, _ = kernel_model(*case)
    assert ok and (n, before) == (16, 2 + extra) and after == 1 + extra
    return case


def width8_case(seed=3):
    """Three topics on 12 brokers in rows of width 8, 2 to 6 replicas each and NONE behind them, leaders skewed as in small_case."""
    rng = np.random.default_rng(seed)
    rows, topic_of = [], []
    for t in range(3):
        for p in range(30):
            rf = int(rng.integers(2, 7))
            rows.append(list(_row(rng, 12, rf, 3, 0.7)) + [NONE] * (8 - rf)); topic_of.append(t)
    rows = np.array(rows, dtype=np.int64)
    assert rows.shape == (90, 8) and (rows[:, 2:] == NONE).any() and (rows[:, 5] != NONE).any() and (rows[:, 6:] == NONE).all()
    return rows, np.array(topic_of, dtype=np.int64), 12, 1, np.zeros(3, dtype=np.int64), np.full(3, 4)
