"""Test-side restatements of kao_failover_order: the follower order that keeps the peak leader count after a
broker or rack failure as low as it can be, with the fewest follower swaps.

  classify          lead[], each partition's scenario, its eligible slots and e(p), straight from the definition
  simulate          {affected, offline, peak} per scenario of rows as they stand (what Kafka would elect), plain numpy
  scenario_optimum  the five reported values per scenario: the HiGHS LP of the flow at a fixed cap M (a network matrix, so the LP
                    value is the integer optimum), M searched upwards from the lower end
  brute_force       the same by enumerating every choice (tiny instances)
  kernel_model      the kernels' probes and phases step by step: output rows, the five values and, on request, the counters
  check_rows        the output rows are the input rows with at most one swap of e(p) and another eligible slot per row
and the instance families of the tests, those on the kernels' dispatch edges at the end.  Rows are [P, width] arrays of dense broker
indices padded with NONE, slot 0 = preferred leader; scope 0 = single-broker failures, 1 = rack failures."""
import functools
import itertools

import numpy as np

NONE = 0xFFFF


def n_scenarios(B, rack_of, scope, n_racks=None):
    if scope == 0:
        return B
    return int(n_racks) if n_racks is not None else int(np.max(rack_of)) + 1


def dead_mask(B, rack_of, scope, g):
    return (np.arange(B) == g) if scope == 0 else (np.asarray(rack_of)[:B] == g)


def classify(rows, B, rack_of, scope):
    """lead[B], scen[P], elig[P, width] (bool; slot 0 never), e[P] (0 = offline)."""
    rows = np.asarray(rows, dtype=np.int64)
    rack_of = np.asarray(rack_of, dtype=np.int64)
    P, W = rows.shape
    lead = np.bincount(rows[:, 0], minlength=B).astype(np.int64)
    scen = rows[:, 0] if scope == 0 else rack_of[rows[:, 0]]
    safe = np.where(rows == NONE, 0, rows)
    group = safe if scope == 0 else rack_of[safe]
    elig = (rows != NONE) & (group != scen[:, None])
    elig[:, 0] = False
    e = np.where(elig.any(axis=1), elig.argmax(axis=1), 0)
    return lead, scen, elig, e


def simulate(rows, B, rack_of, scope, n_racks=None):
    """[n_scen, 3] = affected, offline, peak when every orphaned partition goes to its first live replica."""
    rows = np.asarray(rows, dtype=np.int64)
    lead, scen, elig, e = classify(rows, B, rack_of, scope)
    G = n_scenarios(B, rack_of, scope, n_racks)
    out = np.zeros((G, 3), dtype=np.int64)
    for g in range(G):
        mine = scen == g
        aff = mine & (e > 0)
        alive = ~dead_mask(B, rack_of, scope, g)
        load = lead + np.bincount(rows[aff, e[aff]], minlength=B)
        out[g] = [aff.sum(), (mine & (e == 0)).sum(), load[alive].max() if alive.any() else 0]
    return out


def _scenario_parts(rows, B, rack_of, scope, g, cls):
    lead, scen, elig, e = cls
    aff = np.nonzero((scen == g) & (e > 0))[0]
    alive = ~dead_mask(B, rack_of, scope, g)
    return aff, alive


def _flow_lp(rows, elig, e, aff, lead, M):
    """min #(j != e) s.t. one slot per affected partition, lead[b] + inherit(b) <= M.  None = infeasible."""
    from scipy import sparse
    from scipy.optimize import linprog
    pi, ji = np.nonzero(elig[aff])
    n = len(pi)
    b = rows[aff[pi], ji]
    used, bi = np.unique(b, return_inverse=True)
    cost = (ji != e[aff[pi]]).astype(float)
    a_eq = sparse.csr_matrix((np.ones(n), (pi, np.arange(n))), shape=(len(aff), n))
    a_ub = sparse.csr_matrix((np.ones(n), (bi, np.arange(n))), shape=(len(used), n))
    b_ub = (M - lead[used]).astype(float)
    if (b_ub < 0).any():
        return None
    res = linprog(cost, A_ub=a_ub, b_ub=b_ub, A_eq=a_eq, b_eq=np.ones(len(aff)), bounds=(0, 1), method="highs")
    if res.status == 2:
        return None
    assert res.status == 0, res.message
    value = int(round(res.fun))
    assert abs(res.fun - value) < 1e-6, res.fun
    return value


def lower_end(lead, alive):
    return int(lead[alive].max()) if alive.any() else 0


def scenario_optimum(rows, B, rack_of, scope, n_racks=None):
    """[n_scen, 5] = affected, offline, peak_before, peak_after, reordered."""
    rows = np.asarray(rows, dtype=np.int64)
    cls = classify(rows, B, rack_of, scope)
    lead, scen, elig, e = cls
    sim = simulate(rows, B, rack_of, scope, n_racks)
    out = np.zeros((len(sim), 5), dtype=np.int64)
    for g in range(len(sim)):
        aff, alive = _scenario_parts(rows, B, rack_of, scope, g, cls)
        out[g, :3] = sim[g]
        out[g, 3] = sim[g, 2]
        if len(aff) == 0:
            continue
        for M in range(lower_end(lead, alive), int(sim[g, 2]) + 1):
            swaps = _flow_lp(rows, elig, e, aff, lead, M)
            if swaps is not None:
                out[g, 3], out[g, 4] = M, swaps
                break
        else:
            raise AssertionError("peak_before must be feasible")
    return out


def brute_force(rows, B, rack_of, scope, n_racks=None):
    rows = np.asarray(rows, dtype=np.int64)
    cls = classify(rows, B, rack_of, scope)
    lead, scen, elig, e = cls
    sim = simulate(rows, B, rack_of, scope, n_racks)
    out = np.zeros((len(sim), 5), dtype=np.int64)
    for g in range(len(sim)):
        aff, alive = _scenario_parts(rows, B, rack_of, scope, g, cls)
        out[g, :3] = sim[g]
        out[g, 3] = sim[g, 2]
        if len(aff) == 0:
            continue
        best = None
        for choice in itertools.product(*[np.nonzero(elig[p])[0] for p in aff]):
            load = lead.copy()
            for p, j in zip(aff, choice):
                load[rows[p, j]] += 1
            key = (int(load[alive].max()), sum(int(j != e[p]) for p, j in zip(aff, choice)))
            best = key if best is None or key < best else best
        out[g, 3], out[g, 4] = best
    return out


def check_rows(before, after, B, rack_of, scope):
    """Asserts the output contract row by row; returns the number of rows that changed."""
    before = np.asarray(before, dtype=np.int64)
    after = np.asarray(after, dtype=np.int64)
    assert before.shape == after.shape
    _, _, elig, e = classify(before, B, rack_of, scope)
    assert (before[:, 0] == after[:, 0]).all()
    assert ((before == NONE) == (after == NONE)).all()
    swaps = 0
    for p in np.nonzero((before != after).any(axis=1))[0]:
        d = np.nonzero(before[p] != after[p])[0]
        assert len(d) == 2 and e[p] in d and elig[p, d].all(), (p, before[p], after[p])
        assert before[p, d[0]] == after[p, d[1]] and before[p, d[1]] == after[p, d[0]]
        swaps += 1
    return swaps


# ---- the kernels' algorithm on the host ------------------------------------------------------------------------------------------
K_INF = 0xFFFFFFFF
K_SRC = 1 << 30   # (distance + 2^14) << 16 | arcs


def _solve_model(rows, W, aff, elig, e, lead, alive, M, costed, cur, st=None):
    """One probe at cap M from the start state j = e.  Returns feasible; cur[p] holds the chosen slots.  `st` ([probes, phases,
    rounds, paths, maxlen]) takes the counters as k_fo_solve keeps them: a round is counted up to and including the quiet one; a
    sixth entry, a set, collects the brokers marked as targets (those with room at the smallest distance) over all phases."""
    B = len(lead)
    st = [0] * 5 if st is None else st
    st[0] += 1
    room = np.where(alive, M - lead, 0).astype(np.int64)
    for p in aff:
        cur[p] = e[p]
        room[rows[p, e[p]]] -= 1
    left = int(np.maximum(-room, 0).sum())
    arcs = [(p, j) for p in aff for j in range(1, W) if elig[p, j]]
    while left > 0:
        st[1] += 1
        key = np.where(room < 0, K_SRC, K_INF).astype(np.int64)
        for _ in range(B + 2):
            st[2] += 1
            new = key.copy()
            for p, j in arcs:
                if j == cur[p]:
                    continue
                u, v = rows[p, cur[p]], rows[p, j]
                c = 0 if not costed else (-1 if j == e[p] else (1 if cur[p] == e[p] else 0))
                if key[u] != K_INF and key[u] + c * 65536 + 1 < key[v]:
                    new[v] = min(new[v], key[u] + c * 65536 + 1)
            if (new == key).all():
                break
            key = new
        else:
            raise AssertionError("relaxation did not settle")
        roomy = np.nonzero((room > 0) & (key != K_INF))[0]
        if len(roomy) == 0:
            return False
        dmin = int((key[roomy] >> 16).min())
        if len(st) > 5:
            st[5].update(int(t) for t in roomy if (key[t] >> 16) == dmin)
        pred = {}
        for p, j in arcs:
            if j == cur[p]:
                continue
            u, v = rows[p, cur[p]], rows[p, j]
            c = 0 if not costed else (-1 if j == e[p] else (1 if cur[p] == e[p] else 0))
            if key[u] != K_INF and key[u] + c * 65536 + 1 == key[v]:
                pred[v] = min(pred.get(v, 1 << 40), p * W + j)
        claimed, n = set(), 0
        for t in roomy:
            while room[t] > 0 and (key[t] >> 16) == dmin:
                v, path, ok = t, [], True
                while key[v] & 0xFFFF:
                    a = pred[v]
                    p = a // W
                    if p in claimed:
                        ok = False
                        break
                    path.append(a)
                    v = rows[p, cur[p]]
                if not ok or room[v] >= 0 or len({a // W for a in path}) != len(path):
                    break
                for a in path:
                    cur[a // W] = a % W
                    claimed.add(a // W)
                room[v] += 1
                room[t] -= 1
                n += 1
                st[4] = max(st[4], int(key[t] & 0xFFFF))
        assert n > 0
        st[3] += n
        left -= n
    return True


def kernel_model(rows, B, rack_of, scope, n_racks=None, with_stats=False, targets=None):
    """(output rows, [n_scen, 5]) as the kernels compute them; with_stats adds [scenarios with affected partitions, probes, phases,
    rounds, paths, maxlen] as k_fo_solve accumulates them into ctl[FS_SCEN..FS_MAXLEN]: sums over the scenarios (maxlen: their
    max), a scenario without an affected partition contributing nothing.  A set given as `targets` collects the brokers any phase
    marked as targets."""
    rows = np.asarray(rows, dtype=np.int64)
    W = rows.shape[1]
    cls = classify(rows, B, rack_of, scope)
    lead, scen, elig, e = cls
    sim = simulate(rows, B, rack_of, scope, n_racks)
    out = np.zeros((len(sim), 5), dtype=np.int64)
    cur = e.copy()
    stats = [0] * 6
    for g in range(len(sim)):
        aff, alive = _scenario_parts(rows, B, rack_of, scope, g, cls)
        out[g, :3] = sim[g]
        out[g, 3] = sim[g, 2]
        if len(aff) == 0:
            continue
        st = [0] * 5 + ([] if targets is None else [targets])
        n_alive = int(alive.sum())
        lo = max(lower_end(lead, alive), -(-(int(lead[alive].sum()) + len(aff)) // n_alive))
        hi = int(sim[g, 2])
        while lo < hi:
            mid = (lo + hi) // 2
            if _solve_model(rows, W, aff, elig, e, lead, alive, mid, False, cur, st):
                hi = mid
            else:
                lo = mid + 1
        assert _solve_model(rows, W, aff, elig, e, lead, alive, hi, True, cur, st)
        out[g, 3] = hi
        out[g, 4] = int((cur[aff] != e[aff]).sum())
        stats = [stats[0] + 1] + [a + b for a, b in zip(stats[1:5], st[:4])] + [max(stats[5], st[4])]
    after = rows.copy()
    for p in np.nonzero(cur != e)[0]:
        after[p, e[p]], after[p, cur[p]] = rows[p, cur[p]], rows[p, e[p]]
    return (after, out, stats) if with_stats else (after, out)


# ---- instance families ------------------------------------------------------------------------------------------------------------
def random_instance(rng, B, R, P, W, full=False):
    """Random membership of B brokers in R racks (every rack used when B >= R), rows of 1..W distinct brokers."""
    rack_of = rng.integers(0, R, size=B)
    rack_of[rng.permutation(B)[:min(B, R)]] = np.arange(min(B, R))
    rows = np.full((P, W), NONE, dtype=np.int64)
    for p in range(P):
        k = min(B, W if full else int(rng.integers(1, W + 1)))
        rows[p, :k] = rng.permutation(B)[:k]
    return rows, B, rack_of.astype(np.int64), R


def tiny_family(n=100, seed=11):
    """Instances small enough to enumerate: at most 7 affected partitions per scenario."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        B, R = int(rng.integers(3, 8)), int(rng.integers(1, 4))
        inst = random_instance(rng, B, R, int(rng.integers(3, 16)), int(rng.integers(2, 5)))
        if all(simulate(inst[0], B, inst[2], s, R)[:, 0].max() <= 7 for s in (0, 1)):
            out.append(inst)
    return out


def small_family(n=120, seed=6):
    """3-12 brokers, 1-4 racks with random membership, 4-90 partitions, width 2-4 with each row's length drawn from 1..width."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        B, R = int(rng.integers(3, 13)), int(rng.integers(1, 5))
        P = int(rng.integers(4, 91)) if i % 4 else int(rng.integers(4, 12))
        out.append(random_instance(rng, B, R, P, int(rng.integers(2, 5))))
    return out


@functools.lru_cache(maxsize=None)
def small_family_optima():
    """scenario_optimum of every instance of small_family() in both scopes, computed once per process: [(scope 0, scope 1)]."""
    return [tuple(scenario_optimum(rows, B, rack_of, scope, R) for scope in (0, 1)) for rows, B, rack_of, R in small_family()]


def composition(instances, optima):
    """Counts of the scenario kinds over both scopes, from the reference alone (optima[i][scope] = scenario_optimum): improved,
    unimproved with affected partitions, with offline partitions, peak_after strictly between the lower end and peak_before,
    reordered > peak_before - peak_after, no partition at all."""
    c = dict(improved=0, flat=0, offline=0, between=0, costly=0, empty=0, scenarios=0)
    for (rows, B, rack_of, R), opt in zip(instances, optima):
        for scope in (0, 1):
            lead = classify(rows, B, rack_of, scope)[0]
            for g, (aff, off, before, after, re) in enumerate(opt[scope].tolist()):
                alive = ~dead_mask(B, rack_of, scope, g)
                c["scenarios"] += 1
                c["improved"] += after < before
                c["flat"] += after == before and aff > 0
                c["offline"] += off > 0
                c["between"] += aff > 0 and lower_end(lead, alive) < after < before
                c["costly"] += re > before - after
                c["empty"] += aff == 0 and off == 0
    return c


COMPOSITION_FLOORS = dict(improved=50, flat=50, offline=50, between=50, costly=20, empty=50)


def two_arc_instance():
    """Broker 0 fails.  By order broker 1 inherits p0 and p2 (1 + 2 = 3 leaders), broker 2 inherits p1 (1 + 1 = 2), broker 3
    nothing.  A peak of 2 needs p0 to leave broker 1; its only other replica is on broker 2, which is full at 2 unless p1 moves on
    to broker 3: the one improving path has two arcs."""
    rows = np.array([[0, 1, 2], [0, 2, 3], [0, 1, NONE], [1, 0, NONE], [2, 0, NONE]], dtype=np.int64)
    return rows, 4, np.arange(4, dtype=np.int64), 4


def odd_instance(B=67, seed=2):
    """A broker count that is no multiple of 64; the last broker leads 40 partitions."""
    rng = np.random.default_rng(seed)
    rows, B, rack_of, R = random_instance(rng, B, 5, 400, 4)
    for p in range(40):
        k = int((rows[p] != NONE).sum())
        rows[p, :k] = np.concatenate([[B - 1], rng.permutation(B - 1)[:k - 1]])
    return rows, B, rack_of, R


def many_instance(B=300, R=10, P=9000, seed=3):
    """Leaders p % B, two followers in other racks than the leader's (rack = broker % R)."""
    rng = np.random.default_rng(seed)
    rack_of = np.arange(B) % R
    rows = np.zeros((P, 3), dtype=np.int64)
    rows[:, 0] = np.arange(P) % B
    for p in range(P):
        while True:
            f = rng.integers(0, B, size=2)
            if f[0] != f[1] and rack_of[f[0]] != rack_of[rows[p, 0]] and rack_of[f[1]] != rack_of[rows[p, 0]]:
                break
        rows[p, 1:] = f
    return rows, B, rack_of, R


def limit_instance(B, P=2000, seed=9):
    """40 brokers spread over the whole index range, the last one among them, lead everything and follow each other."""
    rng = np.random.default_rng(seed)
    rack_of = np.arange(B) % 16
    leaders = np.concatenate([[B - 1], rng.permutation(B - 1)[:39]])
    rows = np.array([leaders[rng.permutation(40)[:3]] for _ in range(P)], dtype=np.int64)
    return rows, B, rack_of, 16


# ---- the dispatch edges of the kernels (tests/test_flow_paths_ref.py, tests/test_gpu_failover_paths.py) --------------------------
def lds_bytes(B):
    """Dynamic LDS of a k_fo_solve workgroup: two key buffers, pred and room of 4 bytes per broker, and the bitmap's words."""
    return 16 * B + 4 * ((B + 31) // 32)


def weighted_lds_bytes(B):
    """... of a k_wfo_solve workgroup: load and mark of 8 bytes per broker."""
    return 16 * B


def largest_slots(rows, B, rack_of, scope, n_racks=None):
    """affected partitions of the largest scenario x width: what picks 256 or 1,024 lanes per workgroup (at most 1,024: 256)."""
    return int(simulate(rows, B, rack_of, scope, n_racks)[:, 0].max()) * np.asarray(rows).shape[1]


def hot_leader_instance(n, seed=4):
    """40 brokers in 5 racks (rack = broker % 5), width 4.  Broker 0 leads n partitions of four replicas whose first follower is, four
    times in five, one of the brokers 1, 2, 3, 4, 6; 300 filler rows of 2 to 4 replicas led by the other brokers.  In broker scope
    scenario 0 is the largest by far: n * 4 slots."""
    rng = np.random.default_rng(seed)
    B, R, W = 40, 5, 4
    rows = np.full((n + 300, W), NONE, dtype=np.int64)
    few = np.array([1, 2, 3, 4, 6])
    for p in range(n):
        rest = 1 + rng.permutation(B - 1)[:3]
        if rng.random() < 0.8:
            f = int(few[rng.integers(0, 5)])
            rest = np.concatenate([[f], [b for b in rest if b != f][:2]])
        rows[p] = np.concatenate([[0], rest])
    for p in range(n, n + 300):
        k = int(rng.integers(2, W + 1))
        rows[p, :k] = 1 + rng.permutation(B - 1)[:k]
    rack_of = np.arange(B, dtype=np.int64) % R
    sizes = simulate(rows, B, rack_of, 0, R)[:, 0]
    assert sizes[0] == n and sizes[1:].max() < n and largest_slots(rows, B, rack_of, 0, R) == 4 * n
    return rows, B, rack_of, R


def bitmap_instance(B):
    """Broker 0 leads 2 (B - 2) partitions [0, 1, x], x running twice over 2 .. B - 1, in five racks (rack = broker % 5).  Broker 1
    inherits them all by order, so in scenario 0 every other surviving broker has room at distance 0 and is a target of the first phase:
    brokers 31 and 32 (the last bit of a bitmap word and the first of the next) and B - 1 among them."""
    rows = np.array([[0, 1, 2 + p % (B - 2)] for p in range(2 * (B - 2))], dtype=np.int64)
    rack_of = np.arange(B, dtype=np.int64) % 5
    for scope in (0, 1):
        targets = set()
        kernel_model(rows, B, rack_of, scope, 5, targets=targets)
        assert {31, 32, B - 1} <= targets, sorted(targets)
    return rows, B, rack_of, 5
