"""The restatement of the log-dir balance with exchange moves (tests/logdirs_x_ref.py) against the definition's
own claims, no GPU.  The restatement asserts every round that winners are disjoint, that no replica is touched twice, that the peak
never rises and the sum of squares falls by 2 delta (D - delta) per exchange, that the two candidates are complete (against all
pairs) and that the first exchange round starts from a move-stable state.  Here: the small family ends move-stable and
exchange-stable between the bound, the exhaustive optimum and the plain descent; the counts of brokers at their optimum are pinned;
identity with the plain descent where no exchange exists; order independence; max_rounds and min_gain at their edges; hand-made
cases for y_hi, the tie and the walk."""
import numpy as np
import pytest

import logdirs_ref as lr
import logdirs_x_ref as lx

SEEDS = range(120)
SHARED = ("dir", "n_moved", "bytes_moved", "peak_before", "peak_after", "status")


@pytest.fixture(scope="module")
def small():
    return [(lr.small_case(s), lr.descend(**lr.small_case(s)), lx.descend(**lr.small_case(s))) for s in SEEDS]


def _same_as_plain(x, plain):
    """Every shared field: dir, the numbers, the six shared columns, stats[0..7]; and no exchange round."""
    assert x["dir"].tobytes() == plain["dir"].tobytes() and all(x[k] == plain[k] for k in SHARED[1:])
    assert [p[:6] for p in x["per_broker"]] == plain["per_broker"] and all(p[6:] == [0, 0] for p in x["per_broker"])
    assert x["stats"][:8] == plain["stats"] and x["stats"][8:] == [0, 0, 0, 0]


def test_small_family_stable_between_bound_optimum_and_the_plain_descent(small):
    for c, plain, x in small:   # (the assertions of every round held: descend ran)
        ds, w, bs = c["dir_start"], c["size"], c["base"]
        assert x["stats"][5] == 0 and lr.stable(ds, x["dir"], w, bs) and lx.exchange_stable(ds, x["dir"], w, bs)
        assert int(lr.loads(ds, x["dir"], w, bs).sum()) == int(lr.loads(**c).sum())
        assert [p[2] for p in x["per_broker"]] == lr.lower_bound(**c)
        L = lr.loads(ds, x["dir"], w, bs)
        moved = x["dir"] != c["dir"]
        assert (x["n_moved"], x["bytes_moved"]) == (int(moved.sum()), int(w[moved].sum()))
        for b, (p, q) in enumerate(zip(x["per_broker"], plain["per_broker"])):
            one, mine = lr.one_broker(c, b)
            lo, hi = int(ds[b]), int(ds[b + 1])
            opt = lr.optimum(one["size"], one["base"]) if hi > lo else None
            assert p[1] == int(L[lo:hi].max(initial=0)) and p[0] == q[0] and p[2] == q[2]
            assert p[2] <= (p[1] if opt is None else opt) <= p[1] <= q[1] <= p[0]
            assert p[7] >= p[6] and p[5] - p[6] >= q[5] and (p[6] > 0 or p[5] == q[5])   # the plain call's move rounds come first; an exchange may open further moves


def test_optimum_counts_without_and_with_exchanges(small):
    """The brokers with >= 2 dirs and >= 1 replica that optimum() enumerates: 215; 151 of them end on their optimum without
    exchanges and 194 with; 54 get a lower peak and none a higher one; those above their bound fall from 88 to 77."""
    n = at_plain = at_x = better = worse = above_plain = above_x = 0
    for c, plain, x in small:
        for b, (p, q) in enumerate(zip(x["per_broker"], plain["per_broker"])):
            one, mine = lr.one_broker(c, b)
            if int(c["dir_start"][b + 1] - c["dir_start"][b]) < 2 or len(mine) < 1:
                continue
            opt = lr.optimum(one["size"], one["base"])
            if opt is None:
                continue
            n += 1
            at_plain += q[1] == opt
            at_x += p[1] == opt
            better += p[1] < q[1]
            worse += p[1] > q[1]
            above_plain += q[1] > q[2]
            above_x += p[1] > p[2]
    x_rounds = sum(x["stats"][8] for _, _, x in small)
    print(f"brokers={n} at optimum: {at_plain} -> {at_x}, better={better} worse={worse}, above the bound: {above_plain} -> {above_x}, exchange rounds={x_rounds}")
    assert (n, at_plain, at_x, better, worse, above_plain, above_x, x_rounds) == (215, 151, 194, 54, 0, 88, 77, 92)


def test_larger_instances_come_close_to_their_bound():
    for args, plain_over, x_under in (((4, 4, 40, 0.7, 7), 0.016, 0.0025), ((2, 3, 12, 0.7, 7), 0.054, 0.024)):
        c = lr.lognormal_case(*args)
        plain, x = lr.descend(**c), lx.descend(**c)
        for p, q in zip(x["per_broker"], plain["per_broker"]):
            assert q[1] >= (1 + plain_over) * q[2] and p[1] <= (1 + x_under) * p[2] and p[6] <= p[5] - p[6] + 1


def test_identity_where_no_exchange_exists(small):
    for seed in range(0, 120, 10):   # all sizes 7, or 0
        c, plain, x = small[seed]
        assert set(np.unique(c["size"])) <= {0, 7}
        _same_as_plain(x, plain)
    for n_dirs, k in ((2, 64), (3, 257), (64, 1500), (5, 1)):
        c = lr.crowded_case(n_dirs, k)
        _same_as_plain(lx.descend(**c), lr.descend(**c))
    for c, plain, _ in small[:30]:   # exchange=False is the plain descent
        _same_as_plain(lx.descend(**c, exchange=False), plain)


def test_result_does_not_depend_on_the_order_of_the_replicas():
    """The replicas permuted in the input, the r of their keys permuted with them: the same dir for every replica, the same numbers."""
    for seed in (1, 5, 11, 17, 40, 77, 103):
        c = lr.small_case(seed)
        ref = lx.descend(**c)
        perm = np.random.default_rng(seed).permutation(len(c["dir"]))
        got = lx.descend(c["dir_start"], c["dir"][perm], c["size"][perm], c["base"], ids=perm)
        assert (got["dir"] == ref["dir"][perm]).all() and got["per_broker"] == ref["per_broker"] and got["stats"] == ref["stats"]
    c = lr.lognormal_case(3, 4, 200, 0.7, 5)
    ref = lx.descend(**c)
    perm = np.random.default_rng(5).permutation(len(c["dir"]))
    got = lx.descend(c["dir_start"], c["dir"][perm], c["size"][perm], c["base"], ids=perm)
    assert ref["stats"][8] > 0 and (got["dir"] == ref["dir"][perm]).all() and got["per_broker"] == ref["per_broker"] and got["stats"] == ref["stats"]


def test_max_rounds_cuts_between_the_two_kinds():
    """One broker: cut exactly at the last move round the call is kao_balance_logdirs (with an exchange proposal left); one round more
    applies the first exchange round only."""
    c = lr.lognormal_case(1, 4, 40, 0.7, 7)
    plain, full = lr.descend(**c), lx.descend(**c)
    m = plain["stats"][1]
    assert m > 0 and full["stats"][8] > 1 and full["stats"][1] - full["stats"][8] == m
    cut = lx.descend(**c, max_rounds=m)
    assert cut["dir"].tobytes() == plain["dir"].tobytes() and [p[:6] for p in cut["per_broker"]] == plain["per_broker"]
    assert cut["stats"][:4] == plain["stats"][:4] and cut["stats"][5] == 1 and cut["stats"][8:] == [0, 0, 0, 0]
    one = lx.descend(**c, max_rounds=m + 1)
    assert one["stats"][1] == m + 1 and one["stats"][8] == 1 and one["stats"][9] >= 1 and one["stats"][5] == 1
    assert one["per_broker"][0][5:] == [m + 1, 1, one["stats"][9]]
    changed = np.nonzero(one["dir"] != plain["dir"])[0]
    assert len(changed) == 2 * one["stats"][9]          # an exchange touches two replicas, winners share none
    assert one["peak_after"] <= plain["peak_after"] and lx.descend(**c, max_rounds=10 ** 6)["stats"] == full["stats"]


HAND = dict(dir_start=[0, 2], base=None)   # one broker, two dirs


def _hand(dir, size, **kw):
    return lx.descend(HAND["dir_start"], dir, size, None, **kw)


def test_min_gain_at_a_decisive_gap():
    """L = (21, 17): D = 4, no move (17 + 4 >= 21).  The 10 against the 8 and the 7 against the 5 have delta = 2, D - delta = 2 (their
    y_lo, at the midpoint); they pass iff min_gain < 2, which is min_gain at, just below and just above the decisive D - delta."""
    d, w = [0, 0, 0, 1, 1, 1], [10, 7, 4, 8, 5, 4]
    for mg, n in ((0, 1), (1, 1), (2, 0), (3, 0), (2 ** 64 - 1, 0)):
        r = _hand(d, w, min_gain=mg)
        assert r["stats"][9] == n and r["stats"][8] == n and r["stats"][1] == n, (mg, r["stats"])
        assert lx.exchange_stable(HAND["dir_start"], r["dir"], w, None, mg) and lr.stable(HAND["dir_start"], r["dir"], w, None, mg)
    r = _hand(d, w)
    assert r["dir"].tolist() == [1, 0, 0, 0, 1, 1] and r["per_broker"] == [[21, 19, 19, 2, 18, 1, 1, 1]] and r["status"] == "OPTIMAL_PROVEN"
    assert r["stats"][10] == 2 and r["stats"][11] == 1      # both proposed with delta 2 from the same source: the lower index won


def test_hand_made_y_hi_beats_y_lo():
    """L = (40, 30): D = 10, x = 20: the midpoint is 15, g = the sizes above 15.  On dir 1: 17 (y_hi: delta 3, |6 - 10| = 4) and 11
    (y_lo: delta 9, |18 - 10| = 8): y_hi is taken."""
    d, w = [0, 0, 1, 1, 1], [20, 20, 17, 11, 2]
    r = _hand(d, w, max_rounds=1)
    assert r["stats"][8] == 1 and r["stats"][9] == 1 and r["dir"].tolist() == [1, 0, 0, 1, 1] and r["per_broker"][0][1] == 37


def test_hand_made_tie_goes_to_y_lo():
    """L = (40, 30): D = 10, x = 20: 17 (y_hi: |6 - 10| = 4) and 13 (y_lo: delta 7, |14 - 10| = 4) tie: y_lo, the 13, is taken."""
    d, w = [0, 0, 1, 1], [20, 20, 17, 13]
    r = _hand(d, w, max_rounds=1)
    assert r["stats"][8] == 1 and r["stats"][9] == 1 and r["dir"].tolist() == [1, 0, 1, 0] and r["per_broker"][0][:2] == [40, 37]


def test_hand_made_walk_passes_the_lightest_dir():
    """Three dirs, L = (30, 27, 26), move-stable.  A 10 on dir 0 walks dir 2 first (D = 4): its replicas 13, 13 are larger, no
    partner; then dir 1 (D = 3): a 9 passes (delta 1 < 3), and y_hi, the last 9 of PI, is the partner.  The three 10s propose, the
    lowest index wins."""
    ds, d, w = [0, 3], [0, 0, 0, 1, 1, 1, 2, 2], [10, 10, 10, 9, 9, 9, 13, 13]
    r = lx.descend(ds, d, w, None, max_rounds=1)
    assert r["stats"][:4] == [1, 1, 1, 3] and r["stats"][8:] == [1, 1, 3, 1]
    assert r["dir"].tolist() == [1, 0, 0, 1, 1, 0, 2, 2] and r["per_broker"] == [[30, 29, 28, 2, 19, 1, 1, 1]]


def test_zero_sizes_and_tied_loads_never_exchange():
    r = _hand([0, 0, 1, 1], [6, 0, 0, 4])                      # L = (6, 4): D = 2, the only smaller partner on dir 1 with delta < 2 would be a 5; the 0 never is one
    assert r["stats"][1] == 0 and r["dir"].tolist() == [0, 0, 1, 1]
    r = _hand([0, 0, 1, 1], [6, 4, 7, 3])                      # L = (10, 10): D = 0 is skipped both ways
    assert r["stats"][1] == 0 and r["stats"][10] == 0
