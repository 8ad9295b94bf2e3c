"""Reference for the traffic-weighted leader balance (kao_balance_leaders_weighted), numpy + scipy, no GPU:
a restatement of the synchronous rounds from the text of the definition, the certificate's lower bound, the move-stability check, the
exact optimum by HiGHS (scipy.optimize.milp) and the seeded instance families of the tests.  Loads stay below 2^62, so int64 holds
them; keys are uint64."""
import numpy as np

NONE = 0xFFFF
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def code(t):
    """The monotone 16-bit code of DESIGN.md 4g on an array of values < 2^63: 0 -> 0, else bit length << 9 | the 9 bits below the
    leading one."""
    t = np.asarray(t, dtype=np.uint64)
    e = np.zeros(t.shape, dtype=np.uint64)
    rest = t.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = (rest >> np.uint64(s)) != 0
        e += np.where(big, np.uint64(s), np.uint64(0))
        rest = np.where(big, rest >> np.uint64(s), rest)
    e += (rest != 0).astype(np.uint64)
    safe = np.where(t == 0, np.uint64(1), t)
    es = np.where(t == 0, np.uint64(1), e)
    mant = ((safe << (np.uint64(64) - es)) >> np.uint64(54)) & np.uint64(0x1FF)
    return np.where(t == 0, np.uint64(0), (e << np.uint64(9)) | mant)


def code_scalar(t):
    """The same code on one Python int, bit by bit."""
    if t == 0:
        return 0
    e = t.bit_length()
    return e << 9 | (((t << (64 - e)) & (2 ** 64 - 1)) >> 54) & 0x1FF


def loads(rows, weight, B, lead=None):
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(weight, dtype=np.int64)
    out = np.zeros(B, dtype=np.int64)
    if len(rows):
        leaders = rows[:, 0] if lead is None else rows[np.arange(len(rows)), lead]
        np.add.at(out, leaders, w)
    return out


def descend(rows, weight, B, min_gain=0, max_rounds=0):
    """The rounds of the definition.  Returns a dict: rows (the input rows with slots 0 and j(p) swapped), lead, n_changed,
    peak_before, peak_after, rounds (those that had a proposal), moves, proposals, more (stopped by max_rounds with a proposal left)."""
    rows = np.asarray(rows, dtype=np.int64)
    P = len(rows)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and int(w.sum()) < 2 ** 62
    lead = np.zeros(P, dtype=np.int64)
    W = loads(rows, w, B)
    before = int(W.max()) if B else 0
    rounds = moves = proposals = 0
    more = False
    if P and min_gain < 2 ** 62:
        idx = np.arange(P)
        valid = rows != NONE
        safe = np.where(valid, rows, 0)
        can = (w > 0) & (valid.sum(axis=1) >= 2)
        wcode = np.uint64(0xFFFF) - code(w)
        big = np.int64(2 ** 63 - 1)
        while True:
            seen = np.where(valid, W[safe], big)
            seen[idx, lead] = big
            slot = np.argmin(seen, axis=1)            # the lowest load, ties to the lowest slot index
            a, b = rows[idx, lead], safe[idx, slot]
            Wa, Wb = W[a], seen[idx, slot]
            prop = can & (Wb < big)
            prop &= np.where(prop, Wb, 0) + w + np.int64(min_gain) < Wa
            if not prop.any():
                break
            if max_rounds > 0 and rounds >= max_rounds:
                more = True
                break
            rounds += 1
            proposals += int(prop.sum())
            key = ((np.uint64(0xFFFF) - code(Wa)) << np.uint64(48)) | (wcode << np.uint64(32)) | idx.astype(np.uint64)
            mk = np.full(B, KEY_NONE, dtype=np.uint64)
            np.minimum.at(mk, a[prop], key[prop])
            np.minimum.at(mk, b[prop], key[prop])
            win = prop & (mk[a] == key) & (mk[b] == key)
            assert win.any()                           # the lowest key of all wins
            touched = np.concatenate([a[win], b[win]])
            assert len(np.unique(touched)) == len(touched)   # winners share no broker
            W[a[win]] -= w[win]
            W[b[win]] += w[win]
            lead[win] = slot[win]
            moves += int(win.sum())
    out = rows.copy()
    if P:
        out[np.arange(P), 0], out[np.arange(P), lead] = rows[np.arange(P), lead], rows[np.arange(P), 0]
    return dict(rows=out, lead=lead, n_changed=int((lead != 0).sum()), peak_before=before, peak_after=int(W.max()) if B else 0, rounds=rounds,
                moves=moves, proposals=proposals, more=more, leading=int(len(np.unique(out[:, 0]))) if P else 0)


def lower_bound(rows, weight, B):
    """(bound, k): the certificate from its definition on rows whose slot 0 leads; k = the lowest k that attains the level-set
    term, 0 when that term is below the bound."""
    rows = np.asarray(rows, dtype=np.int64)
    w = [int(x) for x in np.asarray(weight).reshape(-1)]
    W = loads(rows, np.asarray(w, dtype=np.int64), B)
    order = sorted(range(B), key=lambda b: (-int(W[b]), b))
    rank = {b: i for i, b in enumerate(order)}
    hist = [0] * B
    forced = [0] * B
    for r, x in zip(rows.tolist(), w):
        held = [b for b in r if b != NONE]
        hist[max(rank[b] for b in held)] += x
        if len(held) == 1:
            forced[held[0]] += x
    level, level_k, run = 0, 0, 0
    for k in range(1, B + 1):
        run += hist[k - 1]
        v = -(-run // k)
        if v > level:
            level, level_k = v, k
    lb = max([level, max(forced)] + w)
    return lb, (level_k if level == lb else 0)


def stable(rows_in, rows_out, weight, B, min_gain=0):
    """Every output row is its input row with one swap against slot 0, and no partition with weight > 0 has a slot b with
    W(b) + w + min_gain < W(leader)."""
    rin, rout = np.asarray(rows_in, dtype=np.int64), np.asarray(rows_out, dtype=np.int64)
    if rin.shape != rout.shape:
        return False
    for a, b in zip(rin.tolist(), rout.tolist()):
        if a != b:
            j = b.index(a[0]) if a[0] in b else -1
            swapped = list(a)
            if j <= 0 or a[j] == NONE:
                return False
            swapped[0], swapped[j] = a[j], a[0]
            if swapped != b:
                return False
    W = loads(rout, weight, B)
    for r, x in zip(rout.tolist(), [int(v) for v in np.asarray(weight).reshape(-1)]):
        if x > 0 and any(b != NONE and int(W[b]) + x + min_gain < int(W[r[0]]) for b in r[1:]):
            return False
    return True


def optimum(rows, weight, B):
    """The lowest peak any choice of leaders reaches, by HiGHS (scipy.optimize.milp)."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    from scipy.sparse import lil_matrix
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    P = len(rows)
    if P == 0:
        return 0
    var = [(p, j) for p in range(P) for j in range(rows.shape[1]) if rows[p, j] != NONE]
    n = len(var) + 1                                   # the last variable is the peak
    A = lil_matrix((P + B, n))
    for i, (p, j) in enumerate(var):
        A[p, i] = 1
        A[P + rows[p, j], i] = float(w[p])
    for b in range(B):
        A[P + b, n - 1] = -1
    c = np.zeros(n)
    c[-1] = 1
    lo = np.concatenate([np.ones(P), np.full(B, -np.inf)])
    hi = np.concatenate([np.ones(P), np.zeros(B)])
    res = milp(c, constraints=LinearConstraint(A.tocsr(), lo, hi), integrality=np.ones(n), bounds=Bounds(np.zeros(n), np.concatenate([np.ones(n - 1), [np.inf]])))
    assert res.status == 0, res.message
    x = np.round(res.x[:-1])
    lead = np.zeros(P, dtype=np.int64)
    for (p, j), v in zip(var, x):
        if v == 1:
            lead[p] = j
    return int(loads(rows, w, B, lead).max())          # recomputed in integers from the chosen leaders


def skewed_rows(rng, B, P, W, pad=0.0, skew=0.5):
    """P rows of W distinct brokers; a share `pad` of them cut to 1..W-1 replicas; a share `skew` of the rows that hold one of the
    first max(1, B // 4) brokers have it lead."""
    rows = np.full((P, W), NONE, dtype=np.int64)
    hot = max(1, B // 4)
    for p in range(P):
        k = W if rng.random() >= pad else int(rng.integers(1, W))
        r = rng.permutation(B)[:k]
        if rng.random() < skew and (r < hot).any():
            j = int(np.nonzero(r < hot)[0][0])
            r[[0, j]] = r[[j, 0]]
        rows[p, :k] = r
    return rows


def small_case(seed):
    """(rows, weight, B): 3-8 brokers, 6-30 partitions, width 2-4, a third of the rows padded down to one replica; weights 0..49 on
    two seeds of three, log-normal on the third; every tenth seed has all weights equal."""
    rng = np.random.default_rng(1000 + seed)
    B = int(rng.integers(3, 9))
    W = int(rng.integers(2, min(4, B) + 1))
    P = int(rng.integers(6, 31))
    rows = skewed_rows(rng, B, P, W, pad=1 / 3)
    if seed % 10 == 0:
        weight = np.full(P, 7, dtype=np.int64)
    elif seed % 3 == 2:
        weight = np.round(np.exp(rng.normal(4.0, 1.0, P))).astype(np.int64)
    else:
        weight = rng.integers(0, 50, P).astype(np.int64)
    return rows, weight, B


def lognormal_case(B, P, W, sigma, seed):
    """B x P rows of width W, half of them leader-skewed, log-normal weights around 2^20."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, B, (P, W)).astype(np.int64)
    while True:   # redraw the rows that hold a broker twice
        s = np.sort(rows, axis=1)
        bad = np.nonzero((s[:, 1:] == s[:, :-1]).any(axis=1))[0]
        if not len(bad):
            break
        rows[bad] = rng.integers(0, B, (len(bad), W))
    hot = max(1, B // 4)
    for p in np.nonzero(rng.random(P) < 0.5)[0]:
        j = np.nonzero(rows[p] < hot)[0]
        if len(j):
            rows[p, [0, j[0]]] = rows[p, [j[0], 0]]
    weight = np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), sigma, P)))).astype(np.int64)
    return rows, weight


def collide_case(B, P, base=0):
    """Every partition led by broker 0, its other replicas cycling over the rest: all proposals of a round collide at one source.
    weight = base + 5 everywhere when base == 0 (every key ties down to p), else base + a small value."""
    W = min(B, 3)
    rows = np.zeros((P, W), dtype=np.int64)
    for j in range(1, W):
        rows[:, j] = 1 + (np.arange(P) + j - 1) % (B - 1)
    if W == 3 and B == 3:
        rows[:, 2] = 3 - rows[:, 1]
    weight = np.full(P, 5, dtype=np.int64) if base == 0 else base + (np.arange(P) * 7919) % 13
    return rows, weight.astype(np.int64)
