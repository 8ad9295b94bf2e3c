"""Reference for the disk-usage balance with exchange moves (kao_balance_disk_exchange), numpy + plain Python,
no GPU: a restatement of the two kinds of round from the text of the definition, which asserts the definition's own claims every
round, and the brute-force exchange-stability check.  The families, the loads, the admissibility, the rank, the bound, `stable` and
`optimum` are those of tests/disk_ref.py.  Loads stay below 2^62, so int64 holds them; keys are uint64; every reported number is a
Python int.

THE DEFINITION, restated.  PI = the partitions with size > 0 by size descending, then index ascending, fixed for the call.  Rounds are
synchronous on the loads and ranks of their start.  A MOVE round is a round of kao_balance_disk whenever that call has a proposal.
Otherwise the round is an EXCHANGE round: partition x (size > 0) takes its movable slots in ascending rank of their broker; for slot j
on a of rank q it walks c over the ranks B-1 .. q+1; c must be admissible for (x, j) and D = S(a) - S(c) > 0.  M = the members of PI
other than x with a movable slot k on c for which a is admissible.  y passes iff delta = size[x] - size[y] > 0 and delta + min_gain <
D.  The passing members are a contiguous run of M; inside it the split g counts the members with 2 size[y] > 2 size[x] - D; y_hi = the
last passing member before the split, y_lo = the first at or after it, the one with the lower |2 delta - D| is taken, a tie goes to
y_lo.  The first (slot, c) with a passing y is x's proposal, key = q << 48 | (0xFFFF - code(delta)) << 32 | x.  A proposal WINS iff
its key is the lowest of those that touch a, of those that touch c, of those that name x and of those that name y (in either role).
Winners: S(a) -= delta, S(c) += delta, row x[j] = c, row y[k] = a."""
from bisect import bisect_left, bisect_right

import numpy as np

import disk_ref as dr
from wleaders_ref import code

NONE = dr.NONE
KEY_NONE = dr.KEY_NONE
BRUTE_LIMIT = 100   # partitions up to which every exchange round checks COMPLETENESS against all pairs
MASK_WORDS_MAX = 1 << 27   # n_brokers * ceil(N / 64) above this is KAO_ERR_UNSUPPORTED (N = the partitions with size > 0)


def _move_proposals(rows, w, S, order, rank, rk, R, cap, first, mg):
    """The move proposals of kao_balance_disk (disk_ref.descend's round, statement for statement): (best_rank, slot, dest), dest -1 = none."""
    P, W = rows.shape
    B = len(S)
    q = np.arange(B)[None, :]
    held = rows != NONE
    safe = np.where(held, rows, 0)
    best_rank = np.full(P, B, dtype=np.int64)
    slot = np.zeros(P, dtype=np.int64)
    dest = np.full(P, -1, dtype=np.int64)
    for j in range(first, W):
        a = safe[:, j]
        r = rank[a][:, None]
        adm = dr.admissible(rows, rk, R, cap, j)[:, order]
        q1 = dr._first_from_top(adm & (q >= r + 1) & (q <= B - 1 - r))
        q2 = dr._first_from_top(adm & (q >= B - r))
        c = np.full(P, -1, dtype=np.int64)
        for qq in (q2, q1):
            cc = order[np.maximum(qq, 0)]
            ok = (qq >= 0) & (S[a] - S[cc] - w > np.int64(mg))     # S(c) + w + min_gain < S(a), min_gain up to 2^62
            c = np.where(ok, cc, c)
        ok = held[:, j] & (w > 0) & (c >= 0) & (rank[a] < best_rank)
        best_rank = np.where(ok, rank[a], best_rank)
        slot = np.where(ok, j, slot)
        dest = np.where(ok, c, dest)
    return best_rank, slot, dest


def _adm(row, counts, c, rc, ra, cap):
    """c (rack rc) may take a replica of this row (as a list) that leaves rack ra; counts = the row's brokers per rack."""
    return c not in row and (cap <= 0 or rc == ra or counts[rc] < cap)


def _brute_partner(x, j, c, rows, counts, w, rkl, cap, first, D, mg):
    """Does ANY y pass for (x, j, a <-> c)?  Every partition and slot is tried: no index."""
    a = rows[x][j]
    for y in range(len(rows)):
        if y == x or w[y] <= 0:
            continue
        d = w[x] - w[y]
        if not (d > 0 and d < D and D - d > mg):
            continue
        for k in range(first, len(rows[y])):
            if rows[y][k] == c and _adm(rows[y], counts[y], a, rkl[a], rkl[c], cap):
                return True
    return False


def _exchange_proposals(rows_np, w_np, S, order, rank, rk, R, cap, first, mg, pi, pos):
    """The exchange proposals of one round: {x: (j, y, k, a, c, delta, q)}."""
    P, W = rows_np.shape
    B = len(S)
    rows, w, Sl, rkl, ordl, rankl = rows_np.tolist(), w_np.tolist(), S.tolist(), rk.tolist(), order.tolist(), rank.tolist()
    counts = dr.rack_counts(rows_np, rk, R).tolist()
    neg = [-w[p] for p in pi]                                   # PI's sizes, negated: ascending
    members = [[] for _ in range(B)]                            # per broker: the positions of PI with a movable slot on it, ascending
    for t, p in enumerate(pi):
        for j in range(first, W):
            if rows[p][j] != NONE:
                members[rows[p][j]].append(t)
    out = {}
    for x in pi:
        wx = w[x]
        top = bisect_right(neg, -wx)                            # the first position with a size below size[x]: delta > 0 from here on
        found = brute = None
        for q, j in sorted((rankl[rows[x][j]], j) for j in range(first, W) if rows[x][j] != NONE):
            a = rows[x][j]
            for qc in range(B - 1, q, -1):
                c = ordl[qc]
                D = Sl[a] - Sl[c]
                if D <= 0 or not _adm(rows[x], counts[x], c, rkl[c], rkl[a], cap):
                    continue
                if P <= BRUTE_LIMIT and brute is None and _brute_partner(x, j, c, rows, counts, w, rkl, cap, first, D, mg):
                    brute = (j, c)
                if mg >= D:
                    continue
                end = bisect_left(neg, -(wx - (D - mg)))        # the first position with size <= size[x] - D + min_gain
                if end <= top:
                    continue
                mem = members[c]
                M = [t for t in mem[bisect_left(mem, top):bisect_left(mem, end)]                  # the passing run of M, in PI's order
                     if _adm(rows[pi[t]], counts[pi[t]], a, rkl[a], rkl[c], cap)]
                if not M:
                    continue
                assert all(pi[t] != x and 0 < wx - w[pi[t]] < D - mg for t in M)
                g = sum(1 for t in M if 2 * w[pi[t]] > 2 * wx - D)                                # the split, inside the passing run
                assert all(2 * w[pi[t]] > 2 * wx - D for t in M[:g])
                cand = []
                if g < len(M):
                    cand.append((abs(2 * (wx - w[pi[M[g]]]) - D), 0, pi[M[g]]))                   # y_lo; a tie goes to it
                if g > 0:
                    cand.append((abs(2 * (wx - w[pi[M[g - 1]]]) - D), 1, pi[M[g - 1]]))           # y_hi
                y = min(cand)[2]
                k = [k for k in range(first, W) if rows[y][k] == c][0]
                found = (j, y, k, a, c, wx - w[y], q)
                break
            if found:
                break
        if P <= BRUTE_LIMIT:   # COMPLETENESS: the first (slot, c) with any passing y, among ALL partitions, is the proposal's
            assert brute == (None if found is None else (found[0], found[4])), (x, brute, found)
        if found:
            out[x] = found
    return out


def descend(rows, size, B, rack_of, R, cap=0, move_leaders=True, min_gain=0, max_rounds=0, exchange=True):
    """The rounds of the definition.  Returns disk_ref.descend's dict (rounds, moves and proposals count both kinds) and: x_rounds,
    exchanges, x_proposals, x_peak (the peak at the start of the first exchange round, 0 without one), shared (the exchange rounds in
    which two proposals that won at their brokers named one partition), x_lowered (an exchange round lowered the peak), kinds (one
    letter per round that ran: "m" or "x")."""
    rows = np.array(rows, dtype=np.int64)
    start = rows.copy()
    rk = np.asarray(rack_of, dtype=np.int64)
    P, W = rows.shape
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and rk.shape == (B,)
    S = dr.loads(rows, w, B)
    assert int(S.sum()) < 2 ** 62
    S0 = S.copy()
    t = dict(rounds=0, moves=0, proposals=0, more=False, x_rounds=0, exchanges=0, x_proposals=0, x_peak=0, shared=0, x_lowered=False, kinds="")
    ssq = [sum(int(v) ** 2 for v in S)]
    peaks = [int(S.max(initial=0))]
    first = 0 if move_leaders else 1
    mg = min(int(min_gain), 2 ** 62)                            # every gap is below 2^62: nothing passes from there on
    seen_x = False
    if P:
        idx = np.arange(P)
        pi = [int(p) for p in np.lexsort((idx, -w)) if w[p] > 0]
        pos = {p: i for i, p in enumerate(pi)}
        assert B * -(-len(pi) // 64) <= MASK_WORDS_MAX
        wcode = np.uint64(0xFFFF) - code(w)
        while True:
            order, rank = dr.ranking(S)
            best_rank, slot, dest = _move_proposals(rows, w, S, order, rank, rk, R, cap, first, mg)
            prop = dest >= 0
            xp = None
            if exchange and not prop.any():
                if not seen_x:
                    seen_x, t["x_peak"] = True, int(S.max())
                xp = _exchange_proposals(rows, w, S, order, rank, rk, R, cap, first, mg, pi, pos)
            if not prop.any() and not xp:
                break
            if max_rounds > 0 and t["rounds"] >= max_rounds:
                t["more"] = True
                break
            t["rounds"] += 1
            t["kinds"] += "m" if xp is None else "x"
            peak, before = int(S.max()), ssq[-1]
            if xp is None:                                      # ---- a MOVE round: exactly a round of kao_balance_disk
                t["proposals"] += int(prop.sum())
                a = rows[idx, slot]
                key = (best_rank.astype(np.uint64) << np.uint64(48)) | (wcode << np.uint64(32)) | idx.astype(np.uint64)
                mk = np.full(B, KEY_NONE, dtype=np.uint64)
                np.minimum.at(mk, a[prop], key[prop])
                np.minimum.at(mk, dest[prop], key[prop])
                win = prop & (mk[a] == key) & (mk[np.maximum(dest, 0)] == key)
                assert win.any()
                touched = np.concatenate([a[win], dest[win]])
                assert len(np.unique(touched)) == len(touched)
                S[a[win]] -= w[win]
                S[dest[win]] += w[win]
                rows[idx[win], slot[win]] = dest[win]
                t["moves"] += int(win.sum())
            else:                                               # ---- an EXCHANGE round
                t["proposals"] += len(xp)
                t["x_proposals"] += len(xp)
                t["x_rounds"] += 1
                keys = {x: (q << 48) | ((0xFFFF - int(code(np.array([d], dtype=np.int64))[0])) << 32) | x for x, (j, y, k, a, c, d, q) in xp.items()}
                mk, pk = {}, {}
                for x, (j, y, k, a, c, d, q) in xp.items():
                    for word, at in ((mk, a), (mk, c), (pk, x), (pk, y)):
                        word[at] = min(word.get(at, keys[x]), keys[x])
                at_brokers = [x for x, (j, y, k, a, c, d, q) in xp.items() if mk[a] == keys[x] and mk[c] == keys[x]]
                winners = [x for x in at_brokers if pk[x] == keys[x] and pk[xp[x][1]] == keys[x]]
                named = [p for x in at_brokers for p in (x, xp[x][1])]
                t["shared"] += len(set(named)) != len(named)    # without the partition words one row would be written twice
                assert winners and min(keys, key=keys.get) in winners          # the lowest key of all wins: every round applies something
                brokers = [b for x in winners for b in (xp[x][3], xp[x][4])]
                parts = [p for x in winners for p in (x, xp[x][1])]
                assert len(set(brokers)) == len(brokers) and len(set(parts)) == len(parts)   # WINNERS SHARE NO BROKER AND NO PARTITION
                drop = 0
                for x in winners:
                    j, y, k, a, c, d, q = xp[x]
                    D = int(S[a]) - int(S[c])
                    assert rows[x, j] == a and rows[y, k] == c and d == int(w[x]) - int(w[y]) > 0 and d + mg < D
                    drop += 2 * d * (D - d)
                    old = int(S[a])
                    S[a] -= d
                    S[c] += d
                    rows[x, j], rows[y, k] = c, a
                    assert S[a] < old and S[c] < old            # both loads end strictly below the old S(a)
                t["moves"] += len(winners)
                t["exchanges"] += len(winners)
            ssq.append(sum(int(v) ** 2 for v in S))
            peaks.append(int(S.max()))
            assert (S == dr.loads(rows, w, B)).all()                                   # THE LOADS AGREE WITH THE ROWS
            assert ssq[-1] < before and peaks[-1] <= peak                              # THE SUM OF SQUARES FALLS, THE PEAK NEVER RISES
            if xp is not None:
                assert before - ssq[-1] == drop                                        # by 2 delta (D - delta) per exchange
                t["x_lowered"] |= peaks[-1] < peak
            held = [[b for b in r if b != NONE] for r in rows.tolist()]
            assert all(len(set(r)) == len(r) for r in held)                            # NO BROKER TWICE IN A ROW
            assert dr.rack_rule_holds(start, rows, rk, R, cap)
            assert ((rows == NONE) == (start == NONE)).all() and (move_leaders or (rows[:, 0] == start[:, 0]).all())
    n_moved, bytes_moved = dr.set_moves(start, rows, w)
    t.update(rows=rows, n_moved=n_moved, bytes_moved=bytes_moved, peak_before=int(S0.max(initial=0)), peak_after=int(S.max(initial=0)),
             rows_changed=int((rows != start).any(axis=1).sum()) if P else 0, brokers_changed=int((S != S0).sum()), ssq=ssq, peaks=peaks)
    return t


def exchange_stable(rows, size, B, rack_of, R, cap=0, move_leaders=True, min_gain=0):
    """Brute force over every pair of movable slots: no (x, j, a), (y, k, c) with both sides admissible has 0 < delta and
    delta + min_gain < S(a) - S(c), delta = size[x] - size[y], size[y] > 0."""
    rows_np = np.asarray(rows, dtype=np.int64)
    w = [int(v) for v in np.asarray(size).reshape(-1)]
    if min_gain >= 2 ** 62 or not len(rows_np):
        return True
    rkl = [int(v) for v in rack_of]
    S = dr.loads(rows_np, np.asarray(w, dtype=np.int64), B).tolist()
    counts = dr.rack_counts(rows_np, rack_of, R).tolist()
    rows = rows_np.tolist()
    first = 0 if move_leaders else 1
    slots = [(p, j, rows[p][j]) for p in range(len(rows)) if w[p] > 0 for j in range(first, len(rows[p])) if rows[p][j] != NONE]
    for x, j, a in slots:
        for y, k, c in slots:
            d = w[x] - w[y]
            if x == y or d <= 0 or not d + min_gain < S[a] - S[c]:
                continue
            if _adm(rows[x], counts[x], c, rkl[c], rkl[a], cap) and _adm(rows[y], counts[y], a, rkl[a], rkl[c], cap):
                return False
    return True


# ---- hand-built instances (dicts as disk_ref.small_case gives them) ----------------------------------------------------------------
def shared_partner_case():
    """Two proposals that win at their brokers name ONE partition.  The leaders stay (slot 0 is parked on broker 4 or pins a filler), so
    only the followers count.  S = [24, 24, 16, 16, 26] is move-stable.  x1 (p0, follower on 0) finds y's follower on 3; x2 (p1,
    followers on 1 and 3) finds y's follower on 2: four distinct brokers, so both win there, and y (p2) is named twice.  y's word goes
    to the lower key, x1's (rank 1 against rank 2): after one round row y is [4, 2, 0] and x2 has not moved."""
    rows = [[4, 0, NONE], [4, 1, 3], [4, 2, 3], [0, NONE, NONE], [1, NONE, NONE], [2, NONE, NONE]]
    return dict(rows=np.array(rows, dtype=np.int64), size=np.array([10, 10, 6, 14, 14, 10], dtype=np.int64), B=5, rack_of=np.zeros(5, dtype=np.int64), R=1, cap=0,
                move_leaders=False)


def narrow_gain_case():
    """x (p0, size 10) has its follower on broker 0 (S = 29), the followers of y8, y7, y6 (p1..p3) sit on broker 1 (S = 21): D = 8.
    With min_gain = 5 (2 min_gain >= D) delta must be 1 or 2: only y8 passes, and it lies BEFORE the split of all of M (2 size > 12
    holds for y8 and y7), where a bracket around that split looks at y7 and y6 alone and finds nothing.  With min_gain = 0 all three
    pass, the split inside the run is 2, and y6 (|2 * 4 - 8| = 0) is taken."""
    rows = [[2, 0], [2, 1], [2, 1], [2, 1], [0, NONE]]
    return dict(rows=np.array(rows, dtype=np.int64), size=np.array([10, 8, 7, 6, 19], dtype=np.int64), B=3, rack_of=np.zeros(3, dtype=np.int64), R=1, cap=0,
                move_leaders=False)


def rack_partner_case():
    """max_per_rack 1, racks [0, 1, 0, 2].  x (p0, size 10, follower on a = 0, S = 19) looks at c = 1 (S = 11, D = 8).  yA (p1, size 6)
    would be the best partner, but its leader sits on broker 2 in rack(a): a is inadmissible for it.  yB (p2, size 5, leader in rack
    2) is taken.  With max_per_rack 0 it is yA."""
    rows = [[2, 0], [2, 1], [3, 1], [0, NONE], [3, NONE]]
    return dict(rows=np.array(rows, dtype=np.int64), size=np.array([10, 6, 5, 9, 20], dtype=np.int64), B=4, rack_of=np.array([0, 1, 0, 2], dtype=np.int64), R=3, cap=1,
                move_leaders=False)


def leaders_only_case():
    """Width 1: every replica is a slot 0.  With move_leaders the call exchanges x (size 10, on broker 0) with a partition of broker 1;
    without it nothing is movable and the rows stay."""
    rows = [[0], [1], [1], [1], [0]]
    return dict(rows=np.array(rows, dtype=np.int64), size=np.array([10, 8, 7, 6, 19], dtype=np.int64), B=2, rack_of=np.zeros(2, dtype=np.int64), R=1, cap=0,
                move_leaders=True)


def run(c, min_gain=0, max_rounds=0, exchange=True, **over):
    """descend on a case dict; `over` replaces cap / move_leaders."""
    c = dict(c, **over)
    return descend(c["rows"], c["size"], c["B"], c["rack_of"], c["R"], c.get("cap", 0), c.get("move_leaders", True), min_gain, max_rounds, exchange)
