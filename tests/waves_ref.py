"""Reference logic for kao_plan_waves (tests only): an independent checker of a wave split, the sequential first fit in
degree-descending order, a host restatement of the kernel's best-of-orders first fit, of its wave cap and of its order
budget, and the exact optimum of small instances as a HiGHS ILP (scipy.optimize.milp).  Rows are [P, width] dense broker
indices padded with NONE."""
import numpy as np

NONE = 0xFFFF
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def classify(cur, tgt):
    """Per partition: -1 unchanged, 0 changed without an added broker, 1 moving; and the participants of moving ones
    (added brokers + current[p][0])."""
    cls, parts = [], []
    for c, n in zip(np.asarray(cur).tolist(), np.asarray(tgt).tolist()):
        if c == n:
            cls.append(-1)
            parts.append([])
            continue
        cs = {b for b in c if b != NONE}
        add = [b for b in n if b != NONE and b not in cs]
        if not add:
            cls.append(0)
            parts.append([])
            continue
        cls.append(1)
        parts.append(add + ([c[0]] if c[0] != NONE else []))
    return cls, parts


def degrees(parts):
    deg = {}
    for s in parts:
        for b in s:
            deg[b] = deg.get(b, 0) + 1
    return deg


def lower_bound(cur, tgt, k):
    cls, parts = classify(cur, tgt)
    deg = degrees(parts)
    if deg:
        return max(-(-d // k) for d in deg.values())
    return 1 if any(c >= 0 for c in cls) else 0


def check(cur, tgt, k, wave, n_waves, lb):
    """Asserts that (wave, n_waves, lb) is a valid split of the plan under cap k; returns the checker's lower bound."""
    cls, parts = classify(cur, tgt)
    wave = np.asarray(wave).tolist()
    assert len(wave) == len(cls)
    load = {}
    for p, (c, w) in enumerate(zip(cls, wave)):
        if c < 0:
            assert w == -1, (p, w)
        elif c == 0:
            assert w == 0, (p, w)
        else:
            assert 0 <= w < n_waves, (p, w, n_waves)
            for b in parts[p]:
                load[(w, b)] = load.get((w, b), 0) + 1
    assert all(v <= k for v in load.values()), max(load.values())
    used = {w for w in wave if w >= 0}
    assert used == set(range(n_waves)), (sorted(used), n_waves)  # no empty wave
    ref = lower_bound(cur, tgt, k)
    assert lb == ref, (lb, ref)
    assert n_waves >= lb
    return ref


def first_fit(parts, k, order):
    """Sequential first fit of the moving partitions in `order`: wave per partition (-1 for the others)."""
    load = {}
    wave = [-1] * len(parts)
    for p in order:
        w = 0
        while any(load.get((w, b), 0) >= k for b in parts[p]):
            w += 1
        for b in parts[p]:
            load[(w, b)] = load.get((w, b), 0) + 1
        wave[p] = w
    return wave


def degree_order(parts, tie=None):
    """Moving partitions by largest participant degree, descending; ties by `tie(p)` (default: partition index)."""
    deg = degrees(parts)
    mv = [p for p, s in enumerate(parts) if s]
    md = {p: max(deg[b] for b in parts[p]) for p in mv}
    return sorted(mv, key=lambda p: (-md[p], tie(p) if tie else p))


def first_fit_waves(cur, tgt, k):
    """Waves of the sequential first fit in degree-descending order (the kernel's order 0)."""
    cls, parts = classify(cur, tgt)
    w = first_fit(parts, k, degree_order(parts))
    return max(w) + 1 if any(c > 0 for c in cls) else (1 if any(c == 0 for c in cls) else 0)


def _mix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    return x ^ (x >> 16)


def _salt(seed, o):
    z = (seed + 0x9E3779B97F4A7C15 * (o + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return (z ^ (z >> 31)) & M32


def order_fits(cur, tgt, k, seed, n_orders=64):
    """The sequential first fit of each of the kernel's first `n_orders` priority orders: a list of wave-per-partition lists
    (empty when nothing moves)."""
    cls, parts = classify(cur, tgt)
    if not any(c > 0 for c in cls):
        return []
    return [first_fit(parts, k, degree_order(parts, None if o == 0 else (lambda p, s=_salt(seed, o): _mix32(p ^ s))))
            for o in range(n_orders)]


def _best_of(cls, fits, lb, with_winner):
    """The kernel's choice among `fits`: the fewest waves, the lowest order on ties."""
    wave = np.array(cls, dtype=np.int64)
    wave[wave > 0] = -2
    winner = -1
    n_waves = 1 if any(c == 0 for c in cls) else 0
    if fits:
        counts = [max(ww) + 1 for ww in fits]
        winner = counts.index(min(counts))
        n_waves = counts[winner]
        for p, c in enumerate(cls):
            if c > 0:
                wave[p] = fits[winner][p]
    return (wave, n_waves, lb, winner) if with_winner else (wave, n_waves, lb)


def kernel_model(cur, tgt, k, seed, n_orders=64, with_winner=False):
    """What kao_plan_waves computes when it runs `n_orders` orders (order_count; 64 unless the order budget binds):
    (wave, n_waves, lower_bound), and with `with_winner` also the index of the winning order (-1: nothing moves)."""
    return _best_of(classify(cur, tgt)[0], order_fits(cur, tgt, k, seed, n_orders), lower_bound(cur, tgt, k), with_winner)


def wave_cap(cur, tgt, k):
    """The second dimension of the kernel's load array: 1 + max over moving p of the sum over p's participants
    of floor((deg(b) - 1) / k).  0 when nothing moves (the kernel then allocates no loads)."""
    _, parts = classify(cur, tgt)
    deg = degrees(parts)
    return max((1 + sum((deg[b] - 1) // k for b in s) for s in parts if s), default=0)


def order_count(B, wcap, n_mv, sized, k):
    """Orders one call runs (order budget): as many of the 64 as fit 1 GiB of per-order state, at least 1.  Per
    order and (broker, wave): 4 bytes of movement counts (count-only planner, or sized with k >= 1) and 8 bytes of byte loads
    (sized); per order also 4 bytes per moving partition and three 8-byte minimum-key rows over the brokers."""
    per_pair = (4 if (not sized or k > 0) else 0) + (8 if sized else 0)
    per_order = B * wcap * per_pair + 4 * n_mv + 24 * B
    return max(1, min(64, (1 << 30) // per_order))


def ilp_min_waves(cur, tgt, k):
    """Fewest waves, exactly: binary x[p, w] (moving partition p in wave w) and y[w] (wave w used), min sum y, each p in one
    wave, at most k partitions of any broker per wave and only in used waves; waves ordered y[w] >= y[w + 1]."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    cls, parts = classify(cur, tgt)
    mv = [p for p, c in enumerate(cls) if c > 0]
    if not mv:
        return 1 if any(c == 0 for c in cls) else 0
    n_w = first_fit_waves(cur, tgt, k)   # a feasible count: enough waves to choose from
    nx = len(mv) * n_w
    nv = nx + n_w
    rows, lo, hi = [], [], []

    def row(coefs, a, b):
        r = np.zeros(nv)
        for i, v in coefs:
            r[i] += v
        rows.append(r)
        lo.append(a)
        hi.append(b)
    for i in range(len(mv)):
        row([(i * n_w + w, 1) for w in range(n_w)], 1, 1)
    brokers = sorted({b for p in mv for b in parts[p]})
    for b in brokers:
        mine = [i for i, p in enumerate(mv) if b in parts[p]]
        for w in range(n_w):
            row([(i * n_w + w, 1) for i in mine] + [(nx + w, -k)], -np.inf, 0)
    for w in range(n_w - 1):
        row([(nx + w, 1), (nx + w + 1, -1)], 0, np.inf)
    c = np.zeros(nv)
    c[nx:] = 1
    res = milp(c, constraints=LinearConstraint(np.array(rows), lo, hi), integrality=np.ones(nv), bounds=Bounds(0, 1))
    assert res.status == 0, res.message
    return int(round(res.fun))


def random_instance(seed, max_changed=40):
    """A small plan: B brokers, RF 2..4, up to `max_changed` changed partitions (some order-only), k in 1..3."""
    rng = np.random.default_rng(seed)
    rf = int(rng.integers(2, 5))
    B = int(rng.integers(rf + 2, 13))
    P = int(rng.integers(5, max_changed + 1))
    cur = np.array([rng.choice(B, rf, replace=False) for _ in range(P)], dtype=np.uint16)
    tgt = cur.copy()
    for p in range(P):
        r = rng.random()
        if r < 0.15:
            tgt[p] = np.roll(cur[p], 1)                 # leader change only
        elif r < 0.9:
            n_new = int(rng.integers(1, rf + 1))
            free = [b for b in range(B) if b not in cur[p]]
            slots = rng.choice(rf, min(n_new, len(free)), replace=False)
            tgt[p, slots] = rng.choice(free, len(slots), replace=False)
    return cur, tgt, int(rng.integers(1, 4))


def _ids(topic, dense):
    return np.where(dense == NONE, NONE, np.asarray(topic.broker_ids)[np.minimum(dense, len(topic.broker_ids) - 1)]).astype(np.int64)


def config4_pair():
    """BASELINE config 4 as one cluster-wide plan over broker ids 0..549 (the union index: 500 old brokers, 50 of them
    replaced by 500..549).  Current = the config after a 20 % drift, with the replaced brokers still in place; target = the
    balanced fill of the old cluster, every replaced broker swapped for a new broker of its rack."""
    from kafka_assignment_optimizer_amd import synthetic as sy
    topics = sy.make_config(4)
    drifted = sy.drift(topics, 0.2, 1)
    rack0 = np.arange(500) % 10
    target_ids = set(int(b) for b in topics[0].broker_ids)
    gone = sorted(set(range(500)) - target_ids)
    new = sorted(b for b in target_ids if b >= 500)
    by_rack_new = {r: [b for b in new if int(topics[0].rack_of[list(topics[0].broker_ids).index(b)]) == r] for r in range(10)}
    repl = {}
    for r in range(10):
        for i, b in enumerate([g for g in gone if rack0[g] == r]):
            repl[b] = by_rack_new[r][i]
    cur, tgt = [], []
    for ti, (t, d) in enumerate(zip(topics, drifted)):
        old = sy.balanced_fill(500, 10, t.n_partitions, 3, ti, rack0).astype(np.int64)
        c = _ids(d, np.asarray(d.current, dtype=np.int64))
        c = np.where(c == NONE, old, c)                     # slots still on a replaced broker
        cur.append(c)
        tgt.append(np.vectorize(lambda b: repl.get(int(b), int(b)))(old))
    return np.concatenate(cur).astype(np.uint16), np.concatenate(tgt).astype(np.uint16), 550


def drift100k_pair():
    """north_star_topic("drift100k") (1000 brokers x 100,000 partitions RF 3) against a further 20 % drift of it."""
    from kafka_assignment_optimizer_amd import synthetic as sy
    t = sy.north_star_topic("drift100k")
    return (np.asarray(t.current, dtype=np.uint16), np.asarray(sy.drift([t], 0.2, 2)[0].current, dtype=np.uint16), 1000)
