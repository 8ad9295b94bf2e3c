"""The restatement of the disk-usage balance under a byte budget (tests/disk_budget_ref.py) against the
definition's own claims, no GPU: without a budget it is disk_ref.descend; a budget of 0 moves nothing; under a budget the bytes
moved stay inside it, the spend is the set-difference count after every round (asserted inside the restatement), the peak never
rises, the rack rule holds and the end state is stable under what is left.  The Python front end's max_bytes checks are here too."""
import numpy as np
import pytest

import disk_budget_ref as br
import disk_ref as dr

FRACTIONS = (1, 3, 6)   # tenths of the unbudgeted bytes_moved


def _args(c, cap=None):
    return (c["rows"], c["size"], c["B"], c["rack_of"], c["R"], c.get("cap", 0) if cap is None else cap, c.get("move_leaders", True))


def _check_budgeted(c, free, max_bytes, cap=None):
    """One budgeted run held against the claims; returns (the run, the budget binds)."""
    rows, size, B, rack_of, R, cap, ml = _args(c, cap)
    rows = np.asarray(rows, dtype=np.int64)
    ref = br.descend(rows, size, B, rack_of, R, cap, ml, max_bytes=max_bytes)
    assert ref["bytes_moved"] == ref["spent"] <= max_bytes
    assert all(y <= x for x, y in zip(ref["peaks"], ref["peaks"][1:])) and all(y < x for x, y in zip(ref["ssq"], ref["ssq"][1:]))
    assert ref["moves"] >= ref["rounds"] and len(ref["peaks"]) == ref["rounds"] + 1   # every round with a proposal applies a move
    assert dr.rack_rule_holds(rows, ref["rows"], rack_of, R, cap)
    assert ((ref["rows"] == dr.NONE) == (rows == dr.NONE)).all() and (ml or (ref["rows"][:, 0] == rows[:, 0]).all())
    assert br.stable_budget(ref["rows"], rows, size, B, rack_of, R, cap, ml, 0, max_bytes - ref["bytes_moved"])
    assert ref["budget_bound"] == (not dr.stable(ref["rows"], size, B, rack_of, R, cap, ml)) and not ref["more"]
    binds = ref["rows"].tobytes() != free["rows"].tobytes()
    assert binds or not ref["budget_bound"]   # the unbudgeted end state is move-stable
    return ref, binds


def test_small_family():
    binding = refusing = lowering = 0
    for seed in range(120):
        c = dr.small_case(seed)
        rows, size, B, rack_of, R, cap, ml = _args(c)
        plain = dr.descend(rows, size, B, rack_of, R, cap, ml)
        free = br.descend(rows, size, B, rack_of, R, cap, ml)
        assert free["rows"].tobytes() == plain["rows"].tobytes() and free["refused"] == 0 and not free["budget_bound"]
        assert all(free[k] == plain[k] for k in ("rounds", "moves", "proposals", "n_moved", "bytes_moved", "peak_after", "ssq", "peaks"))
        none = br.descend(rows, size, B, rack_of, R, cap, ml, max_bytes=0)
        assert (none["rows"] == np.asarray(rows)).all() and none["moves"] == 0 and none["rounds"] == 0 and none["bytes_moved"] == 0
        assert none["budget_bound"] == (plain["moves"] > 0)
        for tenth in FRACTIONS:
            ref, binds = _check_budgeted(c, free, plain["bytes_moved"] * tenth // 10)
            binding += binds
            refusing += ref["refused"] > 0
            lowering += ref["peak_after"] < ref["peak_before"]
    print(f"of 360 budgeted runs: {binding} bind, {refusing} refuse a winner, {lowering} lower the peak")
    assert binding >= 280 and refusing >= 90 and lowering >= 240   # the family is not vacuous


@pytest.mark.parametrize("B,P,base", [(5, 257, 0), (9, 1500, 2 ** 40)])
def test_contention_shapes(B, P, base):
    c = dr.crowded_case(B, P, base=base)
    rows, size, B, rack_of, R, cap, ml = _args(c)
    plain = dr.descend(rows, size, B, rack_of, R, cap, ml)
    free = br.descend(rows, size, B, rack_of, R, cap, ml)
    assert free["rows"].tobytes() == plain["rows"].tobytes() and (free["rounds"], free["proposals"], free["refused"]) == (plain["rounds"], plain["proposals"], 0)
    for tenth in (1, 5):
        ref, binds = _check_budgeted(c, free, plain["bytes_moved"] * tenth // 10)
        assert binds and ref["budget_bound"] and 0 < ref["bytes_moved"]


def test_two_rounds_by_hand():
    """Brokers 0..3, one rack, sizes 10, 10, 1 on brokers 0, 0, 1: partition 0 moves 0 -> 3 (charge 10, the whole budget) and the loads
    are 10, 1, 0, 10, which no move improves; with a budget of 9 the move is no candidate, and the budget is what stops the descent."""
    rows = np.array([[0], [0], [1]])
    ref = br.descend(rows, [10, 10, 1], 4, np.zeros(4, dtype=np.int64), 1, max_bytes=10)
    assert ref["bytes_moved"] == 10 and ref["moves"] == 1 and ref["peak_after"] == 10 and not ref["budget_bound"]
    tight = br.descend(rows, [10, 10, 1], 4, np.zeros(4, dtype=np.int64), 1, max_bytes=9)
    assert tight["moves"] == 0 and tight["budget_bound"]


def test_front_end_checks_max_bytes_before_the_library_is_loaded(monkeypatch):
    from kafka_assignment_optimizer_amd import _ffi, disk

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_ffi, "load", no_load)
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    for bad in (-1, 2 ** 64, 2 ** 70, 1.5, "7", True):
        with pytest.raises(ValueError, match="max_bytes"):
            disk.balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], max_bytes=bad)
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [0, 1]}]}
    with pytest.raises(ValueError, match="max_bytes"):
        disk.balance_disk(doc, {("t", 0): 5}, broker_list=[0, 1, 2], racks={0: "a", 1: "a", 2: "a"}, max_bytes=-5)
    with pytest.raises(AssertionError, match="loaded"):   # a valid budget gets as far as the library
        disk.balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], max_bytes=2 ** 64 - 1)
    assert disk.BUDGET_STAT_KEYS[8:] == ("refused", "budget_bound") and len(disk.BUDGET_STAT_KEYS) == 10
