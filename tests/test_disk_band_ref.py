"""The restatement of kao_balance_disk_banded (tests/disk_band_ref.py) against the definition, on the CPU: with a
band no count reaches it is disk_ref.descend, and disk_x_ref.descend with exchanges; on the small family with the bands of band_of
the restatement's own assertions hold in every round (winners share no broker, the counts agree with the rows and never leave
[min(lo, n0), max(hi, n0)], the sum of squares falls, the peak never rises), the end is stable inside the band by brute force and, with
exchanges, exchange-stable; with moves only lower_bound <= optimum inside the band <= peak_after <= peak_before, the optimum by HiGHS;
on a count-balanced start an exact band freezes the moves and the exchanges lower the peak at unchanged counts."""
import numpy as np
import pytest

import disk_band_ref as db
import disk_ref as dr
import disk_x_ref as dx

NONE = dr.NONE
SEEDS = range(120)


def _args(c):
    return c["rows"], c["size"], c["B"], c["rack_of"], c["R"]


@pytest.fixture(scope="module")
def family():
    """[(case, band, restatement's result with moves only)] of the 120 seeds, computed once."""
    out = []
    for seed in SEEDS:
        c = dr.small_case(seed)
        band = db.band_of(seed, db.counts(c["rows"], c["B"]))
        out.append((c, band, db.descend_band(*_args(c), band, c["cap"], c["move_leaders"])))
    return out


def test_a_band_no_count_reaches_is_the_plain_descent():
    for seed in SEEDS:
        c = dr.small_case(seed)
        P = len(c["rows"])
        for kw in (dict(), dict(max_rounds=2), dict(min_gain=9)):
            ref = dr.descend(*_args(c), c["cap"], c["move_leaders"], **kw)
            for band in (db.WIDE, (0, P)):
                got = db.descend_band(*_args(c), band, c["cap"], c["move_leaders"], **kw)
                assert got["rows"].tobytes() == ref["rows"].tobytes() and all(got[k] == ref[k] for k in ref if k != "rows")
                assert (got["x_rounds"], got["exchanges"], got["outside_before"], got["outside_after"]) == (0, 0, 0, 0)


def test_a_band_no_count_reaches_is_the_exchange_descent():
    for seed in SEEDS:
        c = dr.small_case(seed)
        for kw in (dict(), dict(max_rounds=3), dict(min_gain=9)):
            ref = dx.descend(*_args(c), c["cap"], c["move_leaders"], **kw)
            got = db.descend_band(*_args(c), (0, len(c["rows"])), c["cap"], c["move_leaders"], exchange=True, **kw)
            assert got["rows"].tobytes() == ref["rows"].tobytes()
            assert all(got[k] == ref[k] for k in ref if k not in ("rows", "shared", "x_lowered"))


def test_bands_are_the_stated_family():
    n0 = np.array([3, 7, 4, 4])
    assert [db.band_of(s, n0) for s in range(4)] == [db.WIDE, (3, 7), (4, 5), (3, 6)]
    assert db.band_of(6, np.array([0, 1, 0])) == (0, 1) and db.band_of(7, np.array([0, 1, 0])) == (0, 2)


def test_small_family_invariants(family):
    moved = frozen = 0
    for c, band, res in family:
        rows, size, B, rack_of, R = _args(c)
        out = res["rows"]
        lo, hi = band
        assert not res["more"] and db.stable_band(out, size, B, rack_of, R, band, c["cap"], c["move_leaders"])
        assert dr.rack_rule_holds(rows, out, rack_of, R, c["cap"]) and ((out == NONE) == (rows == NONE)).all()
        assert c["move_leaders"] or (out[:, 0] == rows[:, 0]).all()
        n0, n = db.counts(rows, B), db.counts(out, B)
        assert (n == res["n"]).all() and (n >= np.minimum(lo, n0)).all() and (n <= np.maximum(hi, n0)).all()
        assert res["count_range"] == (int(n0.min()), int(n0.max()), int(n.min()), int(n.max())) and res["outside_after"] <= res["outside_before"]
        assert res["peak_after"] <= res["peak_before"] and res["x_rounds"] == 0
        moved += res["moves"] > 0
        frozen += res["moves"] < dr.descend(rows, size, B, rack_of, R, c["cap"], c["move_leaders"])["moves"]
    print(f"moved: {moved} of 120, fewer moves than the plain descent: {frozen}")
    assert moved >= 60 and frozen >= 30   # the bands bind, and they leave something to do


def test_small_family_with_exchanges_ends_stable_in_both_senses(family):
    lower = 0
    for c, band, moves in family:
        rows, size, B, rack_of, R = _args(c)
        res = db.descend_band(rows, size, B, rack_of, R, band, c["cap"], c["move_leaders"], exchange=True)
        out = res["rows"]
        assert db.stable_band(out, size, B, rack_of, R, band, c["cap"], c["move_leaders"])
        assert dx.exchange_stable(out, size, B, rack_of, R, c["cap"], c["move_leaders"])
        n0, n = db.counts(rows, B), db.counts(out, B)
        assert (n >= np.minimum(band[0], n0)).all() and (n <= np.maximum(band[1], n0)).all()
        assert res["peak_after"] <= moves["peak_after"]   # (the first exchange round starts at the end state of the moves)
        assert res["x_peak"] in (0, moves["peak_after"])
        lower += res["peak_after"] < moves["peak_after"]
    print(f"exchanges lowered the peak of the moves on {lower} of 120")
    assert lower >= 10


def test_small_family_bound_and_optimum(family):
    at_opt = at_bound = proven = 0
    for c, band, res in family:
        rows, size, B, rack_of, R = _args(c)
        bound, _ = dr.lower_bound(rows, size, B, c["move_leaders"])
        opt = db.optimum_band(rows, size, B, rack_of, R, band, c["cap"], c["move_leaders"], upper=res["peak_after"])
        assert bound <= opt <= res["peak_after"] <= res["peak_before"], (bound, opt, res["peak_after"], res["peak_before"])
        at_opt += res["peak_after"] == opt
        at_bound += bound == opt
        proven += res["peak_after"] == bound
    print(f"peak == optimum: {at_opt}, bound == optimum: {at_bound}, proven: {proven}")
    assert (at_opt, at_bound, proven) == COUNTS   # as measured with this restatement; other counts mean the definition was read differently


COUNTS = (60, 77, 40)


def test_exact_band_on_a_balanced_start():
    """6 brokers, 60 partitions at RF 3, every broker holds 30 replicas: with the band 30..30 no move is admissible, and the exchanges
    lower the peak while every broker keeps its 30."""
    c = db.balanced_case(6, 60, 3, 0.7, 1)
    n0 = db.counts(c["rows"], 6)
    assert n0.tolist() == [30] * 6
    moves = db.run(c, (30, 30))
    assert moves["rounds"] == 0 and (moves["rows"] == c["rows"]).all() and moves["peak_after"] == moves["peak_before"]
    both = db.run(c, (30, 30), exchange=True)
    assert db.counts(both["rows"], 6).tolist() == [30] * 6 and both["count_range"] == (30, 30, 30, 30)
    assert both["exchanges"] > 0 and both["moves"] == both["exchanges"] and both["peak_after"] < both["peak_before"]
    assert dx.exchange_stable(both["rows"], c["size"], 6, c["rack_of"], 1)
    slack = db.run(c, (29, 31), exchange=True)
    n = db.counts(slack["rows"], 6)
    assert n.min() >= 29 and n.max() <= 31 and slack["peak_after"] < moves["peak_before"] and "m" in slack["kinds"]
