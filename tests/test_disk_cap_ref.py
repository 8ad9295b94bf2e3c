"""CPU tests of the disk-usage balance by utilisation (kao_balance_disk_capacity): the restatement in
tests/disk_cap_ref.py lowers the sorted utilisation vector lexicographically in every round, ends move-stable by brute force, needs
THOROUGH rounds on some seeds, is bracketed by the bound and the exact optimum (HiGHS), and with equal capacities is the descent of
tests/disk_ref.py and tests/disk_budget_ref.py move for move; the Python front end checks its capacity arguments."""
from fractions import Fraction

import numpy as np
import pytest

import disk_budget_ref as br
import disk_cap_ref as cr
import disk_ref as dr

NONE = 0xFFFF
SEEDS = range(120)


@pytest.fixture(autouse=True, scope="module")
def bound():
    """The reference restates an entry point: without it there is nothing to hold it against."""
    from kafka_assignment_optimizer_amd import _ffi
    assert "kao_balance_disk_capacity" in _ffi.SIGNATURES
    return _ffi.load().kao_balance_disk_capacity


def _run(c, **kw):
    return cr.descend_cap(c["rows"], c["size"], c["B"], c["rack_of"], c["R"], kw.pop("capacity", c.get("capacity")), kw.pop("cap", c.get("cap", 0)),
                          kw.pop("move_leaders", c.get("move_leaders", True)), **kw)


def test_restatement_falls_lexicographically_ends_stable_and_is_bracketed():
    """On the 120 seeds: the utilisations sorted descending fall lexicographically in every round (so the peak never rises), the end
    state has no admissible move that passes the test, the rack rule holds, lower bound <= optimum <= peak_after as fractions, and
    where proven_cap says proven the peak is the optimum.  At least 8 seeds need a THOROUGH round."""
    need_thorough = proven = at_opt = by_integrality = 0
    for seed in SEEDS:
        c = cr.small_case_cap(seed)
        rows, size, B, rk, R, cap, ml, capv = (c[k] for k in ("rows", "size", "B", "rack_of", "R", "cap", "move_leaders", "capacity"))
        res = _run(c)
        assert len(res["utils"]) == res["rounds"] + 1 and all(y < x for x, y in zip(res["utils"], res["utils"][1:])), seed   # lists compare lexicographically
        assert not res["more"] and not res["budget_bound"] and cr.stable_cap(res["rows"], size, B, rk, R, capv, cap, ml), seed
        assert dr.rack_rule_holds(rows, res["rows"], rk, R, cap), seed
        assert ((res["rows"] == NONE) == (rows == NONE)).all() and (ml or (res["rows"][:, 0] == rows[:, 0]).all()), seed
        assert res["peak_after"] == cr.peak_cap(dr.loads(res["rows"], size, B), capv), seed
        (n, d), term = cr.lower_bound_cap(rows, size, B, capv, ml)
        opt = cr.optimum_cap(rows, size, B, rk, R, capv, cap, ml, upper=res["peak_after"])   # (the end state is a placement: the search starts there)
        assert Fraction(n, d) <= opt <= Fraction(*res["peak_after"]) <= Fraction(*res["peak_before"]), (seed, n, d, opt, res["peak_after"])
        ok, which = cr.proven_cap(res["peak_after"], rows, size, B, capv, ml)
        assert not ok or Fraction(*res["peak_after"]) == opt, (seed, which)
        need_thorough += res["thorough"] > 0
        proven += ok
        by_integrality += ok and which == 3
        at_opt += Fraction(*res["peak_after"]) == opt
    print(f"seeds={len(SEEDS)} need a thorough round: {need_thorough}  peak==optimum: {at_opt}  proven: {proven} (integrality alone: {by_integrality})")
    assert need_thorough >= 8


def test_equal_capacities_are_the_byte_descent():
    """With all capacities equal (1; 12,345; 2^61 / B) the rows, rounds, moves and proposals are those of disk_ref.descend, no round is
    THOROUGH, and the status is the byte planner's; with a finite budget they are those of disk_budget_ref.descend."""
    for seed in SEEDS:
        c = dr.small_case(seed)
        rows, size, B, rk, R, cap, ml = (c[k] for k in ("rows", "size", "B", "rack_of", "R", "cap", "move_leaders"))
        want = dr.descend(rows, size, B, rk, R, cap, ml)
        lb, _ = dr.lower_bound(rows, size, B, ml)
        for common in (1, 12345, 2 ** 61 // B):
            res = _run(c, capacity=[common] * B)
            assert res["rows"].tobytes() == want["rows"].tobytes() and res["thorough"] == 0, (seed, common)
            assert [res[k] for k in ("rounds", "moves", "proposals", "n_moved", "bytes_moved")] == [want[k] for k in ("rounds", "moves", "proposals", "n_moved", "bytes_moved")]
            assert res["peak_before"] == (want["peak_before"], common) and res["peak_after"] == (want["peak_after"], common)
            assert cr.proven_cap(res["peak_after"], rows, size, B, [common] * B, ml)[0] == (want["peak_after"] == lb), (seed, common)
        budget = want["bytes_moved"] * 3 // 10
        capped = br.descend(rows, size, B, rk, R, cap, ml, max_bytes=budget)
        res = _run(c, capacity=[777] * B, max_bytes=budget)
        assert res["rows"].tobytes() == capped["rows"].tobytes() and res["thorough"] == 0, seed
        assert [res[k] for k in ("rounds", "moves", "proposals", "refused", "bytes_moved", "budget_bound")] == \
               [capped[k] for k in ("rounds", "moves", "proposals", "refused", "bytes_moved", "budget_bound")], seed


def test_sum_of_squares_does_not_carry_over():
    """The counter-example of the definition: cap 1 / S 10 -> cap 100 / S 500, size 10 passes the test and raises the sum of S^2."""
    rows = np.array([[0]] + [[1]] * 50)
    size = [10] * 51
    res = cr.descend_cap(rows, size, 2, [0, 0], 1, [1, 100])
    assert res["rows"][0, 0] == 1 and res["moves"] == 1 and res["peak_before"] == (10, 1) and res["peak_after"] == (510, 100)
    assert 510 ** 2 > 10 ** 2 + 500 ** 2


def test_bound_terms_and_integrality():
    rows = np.array([[0, 1], [0, 2], [0, NONE]])
    assert cr.lower_bound_cap(rows, [4, 4, 4], 3, [10, 10, 20], True) == ((20, 40), 1)
    assert cr.lower_bound_cap(rows, [4, 4, 4], 3, [10, 10, 20], False) == ((12, 10), 2)
    assert cr.lower_bound_cap(rows, [9, 1, 1], 3, [10, 10, 10], True) == ((9, 10), 0)
    assert cr.lower_bound_cap(rows, [0, 0, 0], 3, [5, 6, 7], False) == ((0, 7), 0)      # the lowest term on ties
    assert cr.lower_bound_cap(np.zeros((0, 2)), [], 3, [1, 2, 3]) == ((0, 3), 0)
    # three brokers of capacity 1, 7 bytes in units of 1: a peak of 3 is proven by integrality alone (2 + 2 + 2 < 7), 4 is not
    rows = np.array([[0], [0], [0], [1], [1], [2], [2]])
    assert cr.proven_cap((3, 1), rows, [1] * 7, 3, [1, 1, 1]) == (True, 3)
    assert cr.proven_cap((4, 1), rows, [1] * 7, 3, [1, 1, 1]) == (False, 1)
    assert cr.proven_cap((2, 2), np.array([[0], [1], [2]]), [2, 2, 2], 3, [2, 2, 2]) == (True, 0)   # equal to the bound as a fraction


def test_python_front_end_checks_capacity():
    from kafka_assignment_optimizer_amd.disk import balance_disk, balance_disk_arrays, capacity_of
    rows = np.array([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="one capacity per broker"):
        balance_disk_arrays(rows, 3, [0, 0, 0], 1, [1, 2], capacity=[1, 2])
    with pytest.raises(ValueError, match="capacity"):
        balance_disk_arrays(rows, 3, [0, 0, 0], 1, [1, 2], capacity=[1, 0, 2])
    with pytest.raises(ValueError, match="capacity"):
        balance_disk_arrays(rows, 3, [0, 0, 0], 1, [1, 2], capacity=[1, -4, 2])
    with pytest.raises(ValueError, match="2\\^62"):
        balance_disk_arrays(rows, 3, [0, 0, 0], 1, [1, 2], capacity=[2 ** 61, 2 ** 61, 1])
    assert capacity_of([5, 7, 9], {7: 100, 9: "2K"}, 50).tolist() == [50, 100, 2048]
    with pytest.raises(ValueError, match="no capacity for brokers 5, 9 "):
        capacity_of([5, 7, 9], {7: 100})
    assert capacity_of([5, 7], {8: 100, "7": "1M"}, 1).tolist() == [1, 1 << 20]   # a broker outside the list is ignored, as for the racks
    with pytest.raises(ValueError, match="not a byte count"):
        capacity_of([5], {5: 1.5})
    doc = {"version": 1, "partitions": [{"topic": "a", "partition": 0, "replicas": [0, 1]}]}
    with pytest.raises(ValueError, match="no capacity for brokers 2 "):
        balance_disk(doc, {("a", 0): 1}, broker_list=[0, 1, 2], racks={0: "x", 1: "y", 2: "x"}, capacity={0: 10, 1: 10})
