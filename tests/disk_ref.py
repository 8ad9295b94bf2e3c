"""Reference for the disk-usage balance (kao_balance_disk), numpy + scipy, no GPU: a restatement of the
synchronous rounds from the text of the definition, the lower bound, the brute-force move-stability check, the exact optimum by HiGHS
(scipy.optimize.milp) and the seeded instance families of the tests.  Loads stay below 2^62, so int64 holds them; keys are uint64."""
import numpy as np

from wleaders_ref import code

NONE = 0xFFFF
SMALL_BASE = 2000   # (a base whose 120 optima HiGHS proves in about half a minute; some draws of 8 brokers and a near-perfect split take minutes each)
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def loads(rows, size, B):
    """S(b) = the sum of size[p] over the rows that contain b."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    out = np.zeros(B, dtype=np.int64)
    if len(rows):
        held = rows != NONE
        np.add.at(out, rows[held], np.broadcast_to(w[:, None], rows.shape)[held])
    return out


def rack_counts(rows, rack_of, R):
    """[P, R]: the brokers of row p in rack r."""
    rows = np.asarray(rows, dtype=np.int64)
    rk = np.asarray(rack_of, dtype=np.int64)
    out = np.zeros((len(rows), R), dtype=np.int64)
    if len(rows):
        pp, jj = np.nonzero(rows != NONE)
        np.add.at(out, (pp, rk[rows[pp, jj]]), 1)
    return out


def admissible(rows, rack_of, R, cap, j):
    """[P, B] bool: broker c may take the replica in slot j of row p (meaningless for rows whose slot j is empty)."""
    rows = np.asarray(rows, dtype=np.int64)
    rk = np.asarray(rack_of, dtype=np.int64)
    P, B = len(rows), len(rk)
    held = rows != NONE
    in_row = np.zeros((P, B), dtype=bool)
    pp, jj = np.nonzero(held)
    in_row[pp, rows[pp, jj]] = True
    if cap <= 0:
        return ~in_row
    a = np.where(held[:, j], rows[:, j], 0)
    room = rack_counts(rows, rk, R)[:, rk] < cap
    return ~in_row & ((rk[None, :] == rk[a][:, None]) | room)


def ranking(S):
    """(order, rank): the brokers by load descending, ties by index ascending; rank 0 is the heaviest."""
    B = len(S)
    order = np.lexsort((np.arange(B), -S))
    rank = np.empty(B, dtype=np.int64)
    rank[order] = np.arange(B)
    return order, rank


def _first_from_top(mask):
    """Per row of a bool matrix over the ranks: the highest rank that is set, -1 when none is."""
    B = mask.shape[1]
    rev = mask[:, ::-1]
    at = rev.argmax(axis=1)
    return np.where(rev[np.arange(len(mask)), at], B - 1 - at, -1)


def set_moves(rows_in, rows_out, size):
    """(n_moved, bytes_moved): per row the brokers of the final set that the input set did not hold, counted and weighted."""
    n = b = 0
    for x, y, w in zip(np.asarray(rows_in).tolist(), np.asarray(rows_out).tolist(), [int(v) for v in np.asarray(size).reshape(-1)]):
        fresh = len({c for c in y if c != NONE} - {c for c in x if c != NONE})
        n += fresh
        b += fresh * w
    return n, b


def descend(rows, size, B, rack_of, R, cap=0, move_leaders=True, min_gain=0, max_rounds=0):
    """The rounds of the definition.  Returns a dict: rows, n_moved, bytes_moved, peak_before, peak_after, rounds (those that had a
    proposal), moves, proposals, more (stopped by max_rounds with a proposal left), rows_changed, brokers_changed, ssq (the sum of
    S^2 before the first round and after every round, Python ints) and peaks (likewise)."""
    rows = np.array(rows, dtype=np.int64)
    start = rows.copy()
    rk = np.asarray(rack_of, dtype=np.int64)
    P, W = rows.shape
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and rk.shape == (B,)
    S = loads(rows, w, B)
    assert int(S.sum()) < 2 ** 62
    S0 = S.copy()
    ssq = [sum(int(x) ** 2 for x in S)]
    peaks = [int(S.max())]
    rounds = moves = proposals = 0
    more = False
    first = 0 if move_leaders else 1
    if P and min_gain < 2 ** 62:
        idx = np.arange(P)
        q = np.arange(B)[None, :]
        wcode = np.uint64(0xFFFF) - code(w)
        while True:
            order, rank = ranking(S)
            held = rows != NONE
            safe = np.where(held, rows, 0)
            best_rank = np.full(P, B, dtype=np.int64)      # the proposal of the slot whose broker ranks lowest
            slot = np.zeros(P, dtype=np.int64)
            dest = np.full(P, -1, dtype=np.int64)
            for j in range(first, W):
                a = safe[:, j]
                r = rank[a][:, None]
                adm = admissible(rows, rk, R, cap, j)[:, order]   # column = rank
                q1 = _first_from_top(adm & (q >= r + 1) & (q <= B - 1 - r))
                q2 = _first_from_top(adm & (q >= B - r))
                c = np.full(P, -1, dtype=np.int64)
                for qq in (q2, q1):                        # (the first walk's broker wins when both pass)
                    cc = order[np.maximum(qq, 0)]
                    ok = (qq >= 0) & (S[cc] + w + np.int64(min_gain) < S[a])
                    c = np.where(ok, cc, c)
                ok = held[:, j] & (w > 0) & (c >= 0) & (rank[a] < best_rank)
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
            assert win.any()                               # the lowest key of all wins
            touched = np.concatenate([a[win], dest[win]])
            assert len(np.unique(touched)) == len(touched)  # winners share no broker
            S[a[win]] -= w[win]
            S[dest[win]] += w[win]
            rows[idx[win], slot[win]] = dest[win]
            moves += int(win.sum())
            ssq.append(sum(int(x) ** 2 for x in S))
            peaks.append(int(S.max()))
    assert (S == loads(rows, w, B)).all()
    n_moved, bytes_moved = set_moves(start, rows, w)
    return dict(rows=rows, n_moved=n_moved, bytes_moved=bytes_moved, peak_before=int(S0.max()), peak_after=int(S.max()), rounds=rounds, moves=moves,
                proposals=proposals, more=more, rows_changed=int((rows != start).any(axis=1).sum()) if P else 0,
                brokers_changed=int((S != S0).sum()), ssq=ssq, peaks=peaks)


def lower_bound(rows, size, B, move_leaders=True):
    """(bound, term): the maximum of (0) the largest size, (1) the mean load rounded up, (2) with the leaders kept, the largest sum of
    the slot-0 replicas of one broker; term = the one that gives it, the lowest on ties."""
    rows = np.asarray(rows, dtype=np.int64)
    w = [int(x) for x in np.asarray(size).reshape(-1)]
    total = sum(int((r != NONE).sum()) * x for r, x in zip(rows, w))
    fixed = [0] * B
    if not move_leaders:
        for r, x in zip(rows.tolist(), w):
            fixed[r[0]] += x
    terms = [max(w, default=0), -(-total // B), max(fixed)]
    best = max(terms)
    return best, terms.index(best)


def stable(rows, size, B, rack_of, R, cap=0, move_leaders=True, min_gain=0):
    """Brute force over every movable slot and every broker: no admissible move (p, j, a -> c) with size > 0 has
    S(c) + size + min_gain < S(a)."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    if not len(rows) or min_gain >= 2 ** 62:
        return True
    S = loads(rows, w, B)
    for j in range(0 if move_leaders else 1, rows.shape[1]):
        held = (rows[:, j] != NONE) & (w > 0)
        a = np.where(held, rows[:, j], 0)
        gain = S[None, :] + w[:, None] + np.int64(min_gain) < S[a][:, None]
        if (admissible(rows, rack_of, R, cap, j) & gain & held[:, None]).any():
            return False
    return True


def rack_rule_holds(rows_in, rows_out, rack_of, R, cap):
    """No partition's count in a rack is above max(cap, its count there in the input) (no rule with cap <= 0)."""
    return cap <= 0 or bool((rack_counts(rows_out, rack_of, R) <= np.maximum(cap, rack_counts(rows_in, rack_of, R))).all())


def optimum(rows, size, B, rack_of, R, cap=0, move_leaders=True):
    """The lowest peak of any placement the moves could reach, by HiGHS (scipy.optimize.milp): x[p, b] binary, every row keeps its
    replica count, a row's count in a rack is at most max(cap, its input count), slot 0 stays where it is when the leaders are kept.
    Two additions leave the optimum where it is and shorten the proof: the peak is an integer at least max(largest size, mean load)
    (some broker holds the largest partition, one carries the mean) and at most the input's peak (the input is a placement)."""
    from scipy.optimize import Bounds, LinearConstraint, milp
    rows = np.asarray(rows, dtype=np.int64)
    rk = np.asarray(rack_of, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    P = len(rows)
    if P == 0:
        return 0
    n = P * B + 1                                          # the last variable is the peak
    k = (rows != NONE).sum(axis=1)
    cnt = rack_counts(rows, rk, R)
    lb, ub = np.zeros(n), np.ones(n)
    lb[-1] = max(int(w.max()), -(-int((k * w).sum()) // B))
    ub[-1] = int(loads(rows, w, B).max())
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
        if not move_leaders:
            lb[p * B + rows[p, 0]] = 1
        for r in range(R if cap > 0 else 0):
            row([(p * B + b, 1) for b in np.nonzero(rk == r)[0]], 0, max(cap, int(cnt[p, r])))
    for b in range(B):
        row([(p * B + b, float(w[p])) for p in range(P)] + [(n - 1, -1)], -np.inf, 0)
    c = np.zeros(n)
    c[-1] = 1
    res = milp(c, constraints=LinearConstraint(np.array(A), np.array(lo, dtype=float), np.array(hi, dtype=float)), integrality=np.ones(n),
               bounds=Bounds(lb, ub), options={"mip_rel_gap": 0.9 / max(ub[-1], 1.0)})   # peaks are integers: a gap below 1 proves the optimum
    assert res.status == 0, res.message
    x = np.round(res.x[:-1]).reshape(P, B).astype(np.int64)
    assert (x.sum(axis=1) == k).all()
    return int((x * w[:, None]).sum(axis=0).max())         # recomputed in integers from the chosen placement


# ---- the seeded families ---------------------------------------------------------------------------------------------------------
def skewed_rows(rng, B, P, W, pad=0.0):
    """P rows of W distinct brokers drawn without replacement, broker b 1 + 3b / (B - 1) times as likely as broker 0 (a 1:4 skew); a
    share `pad` of the rows cut to 1..W-1 replicas."""
    logp = np.log(1.0 + 3.0 * np.arange(B) / max(B - 1, 1))
    draw = np.argsort(-(logp[None, :] + rng.gumbel(size=(P, B))), axis=1)[:, :W].astype(np.int64)   # Gumbel top-W
    rows = np.full((P, W), NONE, dtype=np.int64)
    rows[:, :] = draw
    if W > 1 and pad > 0:
        cut = rng.random(P) < pad
        k = rng.integers(1, W, P)
        rows[cut[:, None] & (np.arange(W)[None, :] >= k[:, None])] = NONE
    return rows


def small_case(seed):
    """dict(rows, size, B, rack_of, R, cap, move_leaders): 3-8 brokers, 1-4 racks, 6-30 partitions, width 1-4 with a third of the rows
    padded, a tenth of the sizes zero, max_per_rack in {0, 1, 2}, both values of move_leaders."""
    rng = np.random.default_rng(SMALL_BASE + seed)
    B = int(rng.integers(3, 9))
    R = int(rng.integers(1, min(4, B) + 1))
    W = int(rng.integers(1, min(4, B) + 1))
    P = int(rng.integers(6, 31))
    rows = skewed_rows(rng, B, P, W, pad=1 / 3)
    rack_of = np.concatenate([np.arange(R), rng.integers(0, R, B - R)]).astype(np.int64)   # every rack has a broker
    rng.shuffle(rack_of)
    if seed % 10 == 0:
        size = np.full(P, 7, dtype=np.int64)
    elif seed % 3 == 2:
        size = np.round(np.exp(rng.normal(4.0, 1.0, P))).astype(np.int64)
    else:
        size = rng.integers(1, 50, P).astype(np.int64)
    size[rng.random(P) < 0.1] = 0
    return dict(rows=rows, size=size, B=B, rack_of=rack_of, R=R, cap=seed % 3, move_leaders=bool((seed // 3) % 2 == 0))


def lognormal_case(B, R, P, W, sigma, seed, zeros=0.1):
    """dict as small_case (cap and move_leaders left to the caller): skewed placement, racks dealt round-robin, log-normal sizes around
    2^20, a share `zeros` of them zero."""
    rng = np.random.default_rng(seed)
    rows = skewed_rows(rng, B, P, W)
    size = np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), sigma, P)))).astype(np.int64)
    size[rng.random(P) < zeros] = 0
    return dict(rows=rows, size=size, B=B, rack_of=(np.arange(B) % R).astype(np.int64), R=R)


def crowded_case(B, P, W=3, base=0):
    """Every replica on brokers 0..W-1 of B (one rack): all proposals of a round have one of W sources.  size = 5 everywhere when
    base == 0 (every key ties down to p), else base + a small value."""
    rows = (np.arange(W)[None, :] + np.arange(P)[:, None]) % W
    size = np.full(P, 5, dtype=np.int64) if base == 0 else base + (np.arange(P) * 7919) % 13
    return dict(rows=rows.astype(np.int64), size=size.astype(np.int64), B=B, rack_of=np.zeros(B, dtype=np.int64), R=1)
