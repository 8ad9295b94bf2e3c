"""The restatement of kao_balance_disk_drain (tests/disk_drain_ref.py) against the definition, on the CPU: with
no draining broker it is disk_ref.descend; on the small family with the draining sets of drain_of every replica left is stranded, no
move among the live brokers is left, the rack rule holds, nothing arrives on a draining broker, and where nothing is left
lower_bound <= optimum <= peak over the live brokers, the optimum by HiGHS with the draining brokers closed."""
import numpy as np
import pytest

import disk_drain_ref as dd
import disk_ref as dr

NONE = dr.NONE
SEEDS = range(120)


def _args(c):
    return c["rows"], c["size"], c["B"], c["rack_of"], c["R"]


@pytest.fixture(scope="module")
def family():
    """[(case, drain, restatement's result)] of the 120 seeds, computed once."""
    out = []
    for seed in SEEDS:
        c = dr.small_case(seed)
        drain = dd.drain_of(seed, c["B"])
        out.append((c, drain, dd.descend_drain(*_args(c), drain, c["cap"], c["move_leaders"])))
    return out


def _never_arrives(rows_in, rows_out, drain):
    """No replica is on a draining broker that it did not start on (slots keep their place)."""
    rows_in, rows_out = np.asarray(rows_in, dtype=np.int64), np.asarray(rows_out, dtype=np.int64)
    on = (rows_out != NONE) & (np.asarray(drain)[np.where(rows_out != NONE, rows_out, 0)] != 0)
    return bool((rows_out[on] == rows_in[on]).all())


def test_without_a_draining_broker_it_is_the_plain_descent():
    for seed in SEEDS:
        c = dr.small_case(seed)
        for kw in (dict(), dict(max_rounds=2), dict(min_gain=9)):
            ref = dr.descend(*_args(c), c["cap"], c["move_leaders"], **kw)
            got = dd.descend_drain(*_args(c), np.zeros(c["B"], dtype=np.uint8), c["cap"], c["move_leaders"], **kw)
            assert got["rows"].tobytes() == ref["rows"].tobytes() and (got["rounds"], got["proposals"], got["moves"]) == (ref["rounds"], ref["proposals"], ref["moves"])
            assert all(got[k] == ref[k] for k in ref if k != "rows") and (got["n_left"], got["drain_moves"], got["last_drain_round"]) == (0, 0, 0)
        assert dd.lower_bound_drain(c["rows"], c["size"], c["B"], np.zeros(c["B"]), c["move_leaders"]) == dr.lower_bound(c["rows"], c["size"], c["B"], c["move_leaders"])


def test_drain_sets_are_the_stated_family():
    for seed in SEEDS:
        B = dr.small_case(seed)["B"]
        drain = dd.drain_of(seed, B)
        assert drain.shape == (B,) and int(drain.sum()) == (1 if B < 5 else 1 + seed % 2)
        assert sorted(np.nonzero(drain)[0]) == sorted(np.random.default_rng(7000 + seed).choice(B, int(drain.sum()), replace=False))


def test_small_family_invariants(family):
    for c, drain, res in family:
        rows, size, B, rack_of, R = _args(c)
        out = res["rows"]
        assert not res["more"] and dd.left_is_stranded(out, B, rack_of, R, drain, c["cap"])
        assert dd.stable_live(out, size, B, rack_of, R, drain, c["cap"], c["move_leaders"])
        assert dr.rack_rule_holds(rows, out, rack_of, R, c["cap"]) and _never_arrives(rows, out, drain)
        assert ((out == NONE) == (rows == NONE)).all() and int(dr.loads(out, size, B).sum()) == int(dr.loads(rows, size, B).sum())
        on_live = drain[np.where(rows[:, 0] != NONE, rows[:, 0], 0)] == 0
        assert c["move_leaders"] or (out[on_live, 0] == rows[on_live, 0]).all()   # a leader on a live broker stays
        assert (res["n_left"], res["bytes_left"]) == dd.left_on(out, size, drain) and res["n_left"] == len(dd.stranded_reasons(out, B, rack_of, R, drain, c["cap"]))
        assert res["drain_moves"] == res["replicas_left"][0] - res["n_left"] and res["last_drain_round"] <= res["rounds"]
        per_broker = max(int(((rows == b) & (rows != NONE)).sum()) for b in np.nonzero(drain)[0])
        assert res["n_left"] or res["last_drain_round"] >= per_broker   # a draining broker gives up one replica a round


def test_small_family_bound_and_optimum(family):
    done = at_opt = at_bound = proven = 0
    for c, drain, res in family:
        if res["n_left"]:
            continue
        rows, size, B, rack_of, R = _args(c)
        done += 1
        bound, _ = dd.lower_bound_drain(rows, size, B, drain, c["move_leaders"])
        live_peak = int(dr.loads(res["rows"], size, B)[drain == 0].max())
        opt = dd.optimum_drain(rows, size, B, rack_of, R, drain, c["cap"], c["move_leaders"], upper=live_peak)
        assert live_peak == res["peak_after"]                  # the draining brokers are empty
        assert bound <= opt <= live_peak, (bound, opt, live_peak)
        at_opt += live_peak == opt
        at_bound += bound == opt
        proven += live_peak == bound
    print(f"complete: {done} of 120, peak == optimum: {at_opt}, bound == optimum: {at_bound}, proven: {proven}")
    assert done >= 100
    assert (done, at_opt, at_bound, proven) == (105, 46, 55, 21)   # the counts of the definition's prototype; other counts mean it was read differently


def test_optimum_is_confirmed_whatever_bounds_the_peak():
    """Seed 14 (5 brokers, 23 partitions, cap 2, broker 0 draining): with the peak variable bounded by all the bytes HiGHS reports 910
    as proven where 909, the lower bound, is feasible.  The solve one below the candidate finds it."""
    c = dr.small_case(14)
    drain = dd.drain_of(14, c["B"])
    bound, _ = dd.lower_bound_drain(c["rows"], c["size"], c["B"], drain, c["move_leaders"])
    res = dd.descend_drain(*_args(c), drain, c["cap"], c["move_leaders"])
    assert res["n_left"] == 0 and bound == 909 < res["peak_after"]
    assert dd.optimum_drain(*_args(c), drain, c["cap"], c["move_leaders"]) == 909
    assert dd.optimum_drain(*_args(c), drain, c["cap"], c["move_leaders"], upper=res["peak_after"]) == 909


@pytest.mark.parametrize("move_leaders", [True, False])
def test_mid_instance(move_leaders):
    """60 brokers in 6 racks, 1,500 partitions at RF 3, one replica per rack at most, brokers 7, 31 and 59 draining."""
    c = dr.lognormal_case(60, 6, 1500, 3, 0.7, 5)
    rows, size, B, rack_of, R = _args(c)
    drain = dd.drain_flags(B, [7, 31, 59])
    res = dd.descend_drain(rows, size, B, rack_of, R, drain, 1, move_leaders)
    bound, term = dd.lower_bound_drain(rows, size, B, drain, move_leaders)
    print(f"leaders={move_leaders} rounds={res['rounds']} moves={res['moves']} drain_moves={res['drain_moves']} last_drain_round={res['last_drain_round']} "
          f"left={res['n_left']} peak {res['peak_before']} -> {res['peak_after']} bound={bound} term={term} bytes_moved={res['bytes_moved']}")
    out = res["rows"]
    assert res["n_left"] == 0 and res["bytes_left"] == 0 and not res["more"] and res["drain_moves"] == res["replicas_left"][0]
    assert dd.stable_live(out, size, B, rack_of, R, drain, 1, move_leaders) and dr.rack_rule_holds(rows, out, rack_of, R, 1) and _never_arrives(rows, out, drain)
    assert bound <= res["peak_after"] and (dr.loads(out, size, B)[drain != 0] == 0).all()
    assert res["last_drain_round"] >= max(int((rows == b).sum()) for b in (7, 31, 59))
