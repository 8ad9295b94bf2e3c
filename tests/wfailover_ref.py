"""Reference for the traffic-weighted failover order (kao_failover_order_weighted), numpy + scipy, no GPU:

  descend        the synchronous rounds restated from the text of the definition, per scenario and vectorised: output rows, the six
                 values per scenario, the counters
  lower_bound    the certificate from its definition, on rows as they stand (the bound is a function of the returned rows, the
                 weights and the scope alone)
  stable         no move is left on the returned rows
  optimum        the lowest peak of every scenario over all choices: by enumeration (tiny scenarios) or HiGHS (scipy.optimize.milp)
  weights        the seeded weight families
The scenario model (classify, dead_mask, n_scenarios) and the instance families are those of failover_ref, the 16-bit code is the
one of wleaders_ref.  Loads stay below 2^62, so int64 holds them; keys are uint64."""
import itertools

import numpy as np

from failover_ref import NONE, classify, dead_mask, n_scenarios
from wleaders_ref import KEY_NONE, code

SCEN_KEYS = ("affected", "offline", "peak_before", "peak_after", "lower_bound", "reordered")


def wlead(rows, weight, B):
    out = np.zeros(B, dtype=np.int64)
    if len(rows):
        np.add.at(out, np.asarray(rows, dtype=np.int64)[:, 0], np.asarray(weight, dtype=np.int64))
    return out


def _rounds(rows, elig, e, w, aff, load, min_gain, max_rounds):
    """The rounds of one scenario on its affected partitions `aff` (global row indices), loads `load` (changed in place).
    Returns (slot chosen per affected partition, rounds, moves, proposals, more)."""
    r, el = rows[aff], elig[aff]
    n = len(aff)
    idx = np.arange(n)
    cur = e[aff].copy()
    wa = w[aff]
    can = (wa > 0) & (el.sum(axis=1) >= 2)
    safe = np.where(el, r, 0)
    wcode = np.uint64(0xFFFF) - code(wa)
    big = np.int64(2 ** 63 - 1)
    rounds = moves = proposals = 0
    more = False
    if min_gain >= 2 ** 62:
        return cur, 0, 0, 0, False
    while True:
        seen = np.where(el, load[safe], big)
        seen[idx, cur] = big
        slot = np.argmin(seen, axis=1)                 # the lowest load, ties to the lowest slot index
        a, b = r[idx, cur], safe[idx, slot]
        la, lb = load[a], seen[idx, slot]
        prop = can & (lb < big)
        prop &= np.where(prop, lb, 0) + wa + np.int64(min_gain) < la
        if not prop.any():
            break
        if max_rounds > 0 and rounds >= max_rounds:
            more = True
            break
        rounds += 1
        proposals += int(prop.sum())
        key = ((np.uint64(0xFFFF) - code(la)) << np.uint64(48)) | (wcode << np.uint64(32)) | aff.astype(np.uint64)
        mk = np.full(len(load), KEY_NONE, dtype=np.uint64)
        np.minimum.at(mk, a[prop], key[prop])
        np.minimum.at(mk, b[prop], key[prop])
        win = prop & (mk[a] == key) & (mk[b] == key)
        assert win.any()                               # the lowest key of all wins
        touched = np.concatenate([a[win], b[win]])
        assert len(np.unique(touched)) == len(touched)   # winners share no broker
        load[a[win]] -= wa[win]
        load[b[win]] += wa[win]
        cur[win] = slot[win]
        moves += int(win.sum())
    return cur, rounds, moves, proposals, more


def _bound(rows, elig, w, aff, alive, base, load):
    """The certificate of one scenario: base = Wlead, load = the final L_g."""
    if not alive.any():
        return 0
    terms = [int(base[alive].max())]
    if len(aff) == 0:
        return terms[0]
    members = sorted({int(rows[p, j]) for p in aff for j in np.nonzero(elig[p])[0]}, key=lambda b: (-int(load[b]), b))
    rank = {b: i for i, b in enumerate(members)}
    hist = [int(base[b]) for b in members]
    forced = {b: int(base[b]) for b in members}
    for p in aff:
        held = [int(rows[p, j]) for j in np.nonzero(elig[p])[0]]
        terms.append(int(w[p]) + min(int(base[b]) for b in held))
        hist[max(rank[b] for b in held)] += int(w[p])
        if len(held) == 1:
            forced[held[0]] += int(w[p])
    terms.append(max(forced.values()))
    run = 0
    for k in range(1, len(members) + 1):
        run += hist[k - 1]
        terms.append(-(-run // k))
    return max(terms)


def lower_bound(rows, weight, B, rack_of, scope, n_racks=None):
    """[n_scen] the certificate on rows as they stand: the final loads are those of j = e on these rows."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    _, scen, elig, e = classify(rows, B, rack_of, scope)
    base = wlead(rows, w, B)
    out = []
    for g in range(n_scenarios(B, rack_of, scope, n_racks)):
        aff = np.nonzero((scen == g) & (e > 0))[0]
        load = base.copy()
        np.add.at(load, rows[aff, e[aff]], w[aff])
        out.append(_bound(rows, elig, w, aff, ~dead_mask(B, rack_of, scope, g), base, load))
    return out


def descend(rows, weight, B, rack_of, scope, n_racks=None, min_gain=0, max_rounds=0):
    """The definition, scenario by scenario.  Returns a dict: rows (the input rows with e(p) and j(p) swapped), scen ([n_scen][6]
    Python ints, SCEN_KEYS), n_reordered, proven (status OPTIMAL_PROVEN), stats (the eight counters; [4], the launches, is None)."""
    rows = np.asarray(rows, dtype=np.int64)
    P = len(rows)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and int(w.sum()) < 2 ** 62
    _, scen_of, elig, e = classify(rows, B, rack_of, scope)
    base = wlead(rows, w, B)
    G = n_scenarios(B, rack_of, scope, n_racks)
    out = rows.copy()
    scen = []
    st = [0, 0, 0, 0, None, 0, 0, 0]
    for g in range(G):
        mine = scen_of == g
        aff = np.nonzero(mine & (e > 0))[0]
        alive = ~dead_mask(B, rack_of, scope, g)
        load = base.copy()
        np.add.at(load, rows[aff, e[aff]], w[aff])
        before = int(load[alive].max()) if alive.any() else 0
        reordered = 0
        if len(aff):
            cur, rounds, moves, props, more = _rounds(rows, elig, e, w, aff, load, min_gain, max_rounds)
            ch = cur != e[aff]
            p, c, ee = aff[ch], cur[ch], e[aff][ch]
            out[p, ee], out[p, c] = rows[p, c], rows[p, ee]
            reordered = int(ch.sum())
            st[0] += 1; st[1] += rounds; st[2] += moves; st[3] += props; st[5] += int(more); st[7] = max(st[7], rounds)
        after = int(load[alive].max()) if alive.any() else 0
        lb = _bound(rows, elig, w, aff, alive, base, load)
        st[6] += after == lb
        scen.append([len(aff), int((mine & (e == 0)).sum()), before, after, lb, reordered])
    return dict(rows=out, scen=scen, n_reordered=sum(s[5] for s in scen), proven=st[6] == G, stats=st)


def stable(rows_out, weight, B, rack_of, scope, min_gain=0):
    """On the returned rows (whose e(p) is the chosen slot) no affected partition with weight > 0 has an eligible broker b with
    L_g(b) + w + min_gain < L_g(its heir)."""
    rows = np.asarray(rows_out, dtype=np.int64)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    _, scen, elig, e = classify(rows, B, rack_of, scope)
    base = wlead(rows, w, B)
    for g in np.unique(scen[e > 0]):
        aff = np.nonzero((scen == g) & (e > 0))[0]
        load = base.copy()
        np.add.at(load, rows[aff, e[aff]], w[aff])
        for p in aff:
            if w[p] > 0 and any(int(load[rows[p, j]]) + int(w[p]) + min_gain < int(load[rows[p, e[p]]]) for j in np.nonzero(elig[p])[0] if j != e[p]):
                return False
    return True


def _milp_peak(rows, elig, w, aff, base, alive):
    from scipy.optimize import Bounds, LinearConstraint, milp
    from scipy.sparse import lil_matrix
    var = [(i, j) for i, p in enumerate(aff) for j in np.nonzero(elig[p])[0]]
    used = sorted({int(rows[aff[i], j]) for i, j in var})
    at = {b: k for k, b in enumerate(used)}
    n, na, nb = len(var) + 1, len(aff), len(used)
    A = lil_matrix((na + nb, n))
    for v, (i, j) in enumerate(var):
        A[i, v] = 1
        A[na + at[int(rows[aff[i], j])], v] = float(w[aff[i]])
    for k in range(nb):
        A[na + k, n - 1] = -1
    c = np.zeros(n)
    c[-1] = 1
    lo = np.concatenate([np.ones(na), np.full(nb, -np.inf)])
    hi = np.concatenate([np.ones(na), [-float(base[b]) for b in used]])
    res = milp(c, constraints=LinearConstraint(A.tocsr(), lo, hi), integrality=np.ones(n), bounds=Bounds(np.zeros(n), np.concatenate([np.ones(n - 1), [np.inf]])))
    assert res.status == 0, res.message
    load = base.copy()
    chosen = np.zeros(na, dtype=np.int64)
    for (i, j), x in zip(var, np.round(res.x[:-1])):
        if x == 1:
            chosen[i] = j
    assert (chosen > 0).all()
    np.add.at(load, rows[aff, chosen], w[aff])
    return int(load[alive].max())                      # recomputed in integers from the chosen slots


def optimum(rows, weight, B, rack_of, scope, n_racks=None, enumerate_up_to=7):
    """[n_scen] the lowest peak_g any choice of slots reaches: every choice tried when the scenario has at most `enumerate_up_to`
    affected partitions, else HiGHS."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(weight, dtype=np.int64).reshape(-1)
    _, scen, elig, e = classify(rows, B, rack_of, scope)
    base = wlead(rows, w, B)
    out = []
    for g in range(n_scenarios(B, rack_of, scope, n_racks)):
        aff = np.nonzero((scen == g) & (e > 0))[0]
        alive = ~dead_mask(B, rack_of, scope, g)
        if len(aff) == 0:
            out.append(int(base[alive].max()) if alive.any() else 0)
        elif len(aff) <= enumerate_up_to:
            best = None
            for choice in itertools.product(*[np.nonzero(elig[p])[0] for p in aff]):
                load = base.copy()
                for p, j in zip(aff, choice):
                    load[rows[p, j]] += w[p]
                peak = int(load[alive].max())
                best = peak if best is None or peak < best else best
            out.append(best)
        else:
            out.append(_milp_peak(rows, elig, w, aff, base, alive))
    return out


# ---- weight families ----------------------------------------------------------------------------------------------------------------
def family_weights(i, P, seed=500):
    """Weights of instance i of a family: integers 0..49 on even i, a rounded log-normal (median e^4, sigma 1) on odd i."""
    rng = np.random.default_rng(seed + i)
    if i % 2 == 0:
        return rng.integers(0, 50, P).astype(np.int64)
    return np.round(np.exp(rng.normal(4.0, 1.0, P))).astype(np.int64)


def lognormal_weights(P, sigma, seed):
    """Log-normal weights around 2^20, at least 1, as in section 4k."""
    rng = np.random.default_rng(seed)
    return np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), sigma, P)))).astype(np.int64)


def contention_case(B, P, base=0):
    """(rows, weight, B, rack_of, n_racks), B >= 3, width 3: every partition is led by broker 0 and elects broker 1 first, its
    other follower cycles over the brokers from 2 on.  In broker scope scenario 0 holds all P partitions and every proposal of the
    first rounds leaves broker 1.  weight = 5 everywhere when base == 0 (every key ties down to p), else base + a small value."""
    rows = np.zeros((P, 3), dtype=np.int64)
    rows[:, 1] = 1
    rows[:, 2] = 2 + np.arange(P) % (B - 2)
    weight = np.full(P, 5, dtype=np.int64) if base == 0 else base + (np.arange(P) * 7919) % 13
    return rows, weight.astype(np.int64), B, np.arange(B) % 2, 2
