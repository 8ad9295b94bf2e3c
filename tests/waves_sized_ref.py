"""Reference logic for kao_plan_waves_sized (tests only): traffic per participant, an independent checker of a byte-capped wave
split, the sequential first fit under both caps, a host restatement of the kernel's priority orders (bit for bit) and of its wave cap, the exact
optimum of small instances as a HiGHS ILP, and a deterministic heavy-tailed size generator.  Rows as in waves_ref."""
import numpy as np

from waves_ref import (M32, NONE, _best_of, _mix32, _salt, classify, config4_pair, drift100k_pair, order_count,  # noqa: F401
                       random_instance)

LIMIT = 1 << 62


def traffic(cur, tgt, size):
    """(cls, parts, traf): classify's classes and participants, and traf[p][j] = bytes participant parts[p][j] moves --
    size[p] at an added broker, n_added(p) * size[p] at the source (the last participant when current[p][0] is a broker)."""
    cls, parts = classify(cur, tgt)
    traf = []
    cur = np.asarray(cur)
    for p, s in enumerate(parts):
        if not s:
            traf.append([])
            continue
        n_added = len(s) - 1 if cur[p][0] != NONE else len(s)
        sz = int(size[p])
        traf.append([sz if j < n_added else n_added * sz for j in range(len(s))])
    return cls, parts, traf


def totals(parts, traf, C=0):
    """Per broker: T_b = sum of t_p(b), and sum of min(t_p(b), C)."""
    tot, clamp = {}, {}
    for s, ts in zip(parts, traf):
        for b, t in zip(s, ts):
            tot[b] = tot.get(b, 0) + t
            clamp[b] = clamp.get(b, 0) + min(t, C)
    return tot, clamp


def lower_bound_sized(cur, tgt, size, C, k):
    cls, parts, traf = traffic(cur, tgt, size)
    if not any(c > 0 for c in cls):
        return 1 if any(c == 0 for c in cls) else 0
    deg = {}
    for s in parts:
        for b in s:
            deg[b] = deg.get(b, 0) + 1
    lb = 1   # a moving partition needs a wave, whatever its size
    if k:
        lb = max(-(-d // k) for d in deg.values())
    if C:
        _, clamp = totals(parts, traf, C)
        lb = max(lb, max(-(-v // C) for v in clamp.values()))
    return lb


def check_sized(cur, tgt, size, C, k, wave, n_waves, lb):
    """Asserts that (wave, n_waves, lb) is a valid byte-capped split: coverage, wave -1 / 0 classes, at most k movements per
    broker per wave (k >= 1), bytes per broker per wave <= C unless exactly one partition with nonzero traffic there (the
    oversize rule; C >= 1), no empty wave, and the exact lower bound.  Returns the lower bound."""
    cls, parts, traf = traffic(cur, tgt, size)
    wave = np.asarray(wave).tolist()
    assert len(wave) == len(cls)
    cnt, byt, pos = {}, {}, {}
    for p, (c, w) in enumerate(zip(cls, wave)):
        if c < 0:
            assert w == -1, (p, w)
        elif c == 0:
            assert w == 0, (p, w)
        else:
            assert 0 <= w < n_waves, (p, w, n_waves)
            for b, t in zip(parts[p], traf[p]):
                cnt[(w, b)] = cnt.get((w, b), 0) + 1
                byt[(w, b)] = byt.get((w, b), 0) + t
                pos[(w, b)] = pos.get((w, b), 0) + (t > 0)
    if k:
        assert all(v <= k for v in cnt.values()), max(cnt.values())
    if C:
        bad = [(key, v, pos[key]) for key, v in byt.items() if v > C and pos[key] != 1]
        assert not bad, bad[:5]
    used = {w for w in wave if w >= 0}
    assert used == set(range(n_waves)), (sorted(used), n_waves)
    ref = lower_bound_sized(cur, tgt, size, C, k)
    assert lb == ref, (lb, ref)
    assert n_waves >= lb
    return ref


def first_fit_sized(parts, traf, C, k, order):
    """Sequential first fit in `order` under the kernel's fit test: count < k (k >= 1) and, at every participant,
    load == 0 or load + t <= C (C >= 1)."""
    cnt, byt = {}, {}
    wave = [-1] * len(parts)
    for p in order:
        w = 0
        while True:
            fit = True
            for b, t in zip(parts[p], traf[p]):
                if k and cnt.get((w, b), 0) >= k:
                    fit = False
                l = byt.get((w, b), 0)
                if C and not (l == 0 or l + t <= C):
                    fit = False
            if fit:
                break
            w += 1
        for b, t in zip(parts[p], traf[p]):
            cnt[(w, b)] = cnt.get((w, b), 0) + 1
            byt[(w, b)] = byt.get((w, b), 0) + t
        wave[p] = w
    return wave


def bytes_code(t):
    """The kernel's monotone 16-bit code of a byte count: 0 -> 0, else bit length e << 9 | the 9 bits below the leading one."""
    if t == 0:
        return 0
    e = t.bit_length()
    return e << 9 | ((t << (64 - e)) & ((1 << 64) - 1)) >> 54 & 0x1FF


def key_high(parts, traf):
    """Per moving partition: the key's high word, (0xFFFF - code(max t)) << 16 | (0xFFFF - min(max degree, 0xFFFF))."""
    deg = {}
    for s in parts:
        for b in s:
            deg[b] = deg.get(b, 0) + 1
    return {p: (0xFFFF - bytes_code(max(traf[p]))) << 16 | (0xFFFF - min(max(deg[b] for b in s), 0xFFFF))
            for p, s in enumerate(parts) if s}


def sized_order(parts, traf, o=0, seed=1):
    """Order o of the kernel: ascending (key_high << 32 | tie), tie = p (o = 0) or mix32(p ^ salt(seed, o))."""
    hi = key_high(parts, traf)
    salt = _salt(seed, o)
    return sorted(hi, key=lambda p: hi[p] << 32 | (p if o == 0 else _mix32(p ^ salt)))


def first_fit_sized_waves(cur, tgt, size, C, k):
    """Waves of the kernel's order 0 run sequentially: first fit decreasing by traffic."""
    cls, parts, traf = traffic(cur, tgt, size)
    if not any(c > 0 for c in cls):
        return 1 if any(c == 0 for c in cls) else 0
    return max(first_fit_sized(parts, traf, C, k, sized_order(parts, traf))) + 1


def order_fits_sized(cur, tgt, size, C, k, seed, n_orders=64):
    """The sequential first fit of each of the kernel's first `n_orders` priority orders (empty when nothing moves)."""
    cls, parts, traf = traffic(cur, tgt, size)
    if not any(c > 0 for c in cls):
        return []
    return [first_fit_sized(parts, traf, C, k, sized_order(parts, traf, o, seed)) for o in range(n_orders)]


def kernel_model_sized(cur, tgt, size, C, k, seed, n_orders=64, with_winner=False):
    """What kao_plan_waves_sized computes when it runs `n_orders` orders (order_count; 64 unless the order budget binds):
    (wave, n_waves, lower_bound), and with `with_winner` also the index of the winning order (-1: nothing moves)."""
    return _best_of(classify(cur, tgt)[0], order_fits_sized(cur, tgt, size, C, k, seed, n_orders),
                    lower_bound_sized(cur, tgt, size, C, k), with_winner)


def wave_cap_sized(cur, tgt, size, C, k):
    """The second dimension of the kernel's load arrays: 1 + max over moving p of the sum over p's participants
    b of the waves that can be blocked at b ahead of p's -- by count floor((deg(b) - 1) / k) (k >= 1), by bytes at most
    min(deg(b) - 1, by) (C >= 1), where the other partitions at b carry rest = T_b - t_p(b) bytes and by = rest when
    t_p(b) > C (every nonzero load blocks), floor(rest / (C - t_p(b) + 1)) when a blocking load (> C - t_p(b)) fits into rest at
    all, else 0.  0 when nothing moves."""
    _, parts, traf = traffic(cur, tgt, size)
    tot, _ = totals(parts, traf)
    deg = {}
    for s in parts:
        for b in s:
            deg[b] = deg.get(b, 0) + 1
    cap = 0
    for s, ts in zip(parts, traf):
        if not s:
            continue
        blocked = 0
        for b, t in zip(s, ts):
            if k >= 1:
                blocked += (deg[b] - 1) // k
            if C >= 1:
                rest = tot[b] - t
                if t > C:
                    by = rest
                elif C - t < rest:
                    by = rest // (C - t + 1)
                else:
                    by = 0
                blocked += min(deg[b] - 1, by)
        cap = max(cap, 1 + blocked)
    return cap


def ilp_min_waves_sized(cur, tgt, size, C, k):
    """Fewest waves, exactly: binary x[p, w], y[w]; each p in one wave; count rows sum x <= k y (k >= 1); byte rows
    sum min(t, C) x <= C y (C >= 1: a partition above C at b counts C there, so it is alone among the nonzero ones, which is
    the checker's oversize rule); waves ordered y[w] >= y[w + 1]."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    cls, parts, traf = traffic(cur, tgt, size)
    mv = [p for p, c in enumerate(cls) if c > 0]
    if not mv:
        return 1 if any(c == 0 for c in cls) else 0
    n_w = first_fit_sized_waves(cur, tgt, size, C, k)
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
        mine = [(i, traf[p][parts[p].index(b)]) for i, p in enumerate(mv) if b in parts[p]]
        for w in range(n_w):
            if k:
                row([(i * n_w + w, 1) for i, _ in mine] + [(nx + w, -k)], -np.inf, 0)
            if C:   # scaled by C so that the coefficients stay near 1
                row([(i * n_w + w, min(t, C) / C) for i, t in mine] + [(nx + w, -1)], -np.inf, 1e-9)
    for w in range(n_w - 1):
        row([(nx + w, 1), (nx + w + 1, -1)], 0, np.inf)
    c = np.zeros(nv)
    c[nx:] = 1
    # presolve off: HiGHS's presolve has declared feasible instances with coefficients spanning six decades infeasible
    res = milp(c, constraints=LinearConstraint(np.array(rows), lo, hi), integrality=np.ones(nv), bounds=Bounds(0, 1),
               options={"presolve": False})
    assert res.status == 0, res.message
    return int(round(res.fun))


def gen_sizes(n, seed, zero_share=0.1, lo=1 << 10, hi=1 << 40):
    """n partition sizes, log-uniform from 1 KiB to 1 TiB, a share of them 0 (empty partitions); deterministic in seed."""
    rng = np.random.default_rng(seed)
    s = np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.uint64)
    s[rng.random(n) < zero_share] = 0
    return s


def random_sized_instance(seed, max_changed=40):
    """random_instance's plan with generated sizes, a byte cap C around the typical traffic (or none) and k in 0..3."""
    cur, tgt, k = random_instance(seed, max_changed)
    size = gen_sizes(cur.shape[0], seed + 1000)
    _, parts, traf = traffic(cur, tgt, size)
    ts = sorted(t for tt in traf for t in tt if t > 0)
    rng = np.random.default_rng(seed + 2000)
    C = int(ts[int(rng.integers(0, len(ts)))]) * int(rng.integers(1, 4)) if ts else 1
    if seed % 3 == 0:
        k = 0
    return cur, tgt, size, C, k
