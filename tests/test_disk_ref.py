"""CPU tests of the disk-usage balance (kao_balance_disk): the restatement of the rounds in tests/disk_ref.py
ends, never raises the peak, lowers the sum of squared loads in every round, ends move-stable, keeps the rack rule and is bracketed
by the lower bound and the exact optimum (HiGHS) on the small family; the contention and rack shapes of the GPU tests behave as
their docstrings say; the Python front end checks its arguments."""
import numpy as np
import pytest

import disk_ref as dr

NONE = 0xFFFF
SEEDS = range(120)


@pytest.fixture(autouse=True, scope="module")
def bound():
    """The reference restates an entry point: without it there is nothing to hold it against."""
    from kafka_assignment_optimizer_amd import _ffi
    assert "kao_balance_disk" in _ffi.SIGNATURES
    return _ffi.load().kao_balance_disk


def _run(c, **kw):
    return dr.descend(c["rows"], c["size"], c["B"], c["rack_of"], c["R"], kw.pop("cap", c.get("cap", 0)),
                      kw.pop("move_leaders", c.get("move_leaders", True)), **kw)


def test_restatement_is_stable_and_bracketed_on_the_small_family():
    """lower_bound <= optimum <= peak_after <= peak_before on 120 seeds; the sum of S^2 falls strictly in every round and the peak
    never rises; the descent ends with no move left; no rack count passes max(cap, input).  How often the descent reaches the
    optimum and how often the bound does is printed: a measurement, not a requirement."""
    at_opt = lb_at_opt = proven = moved = padded = kept = capped = zeros = 0
    for seed in SEEDS:
        c = dr.small_case(seed)
        rows, size, B, rk, R, cap, ml = (c[k] for k in ("rows", "size", "B", "rack_of", "R", "cap", "move_leaders"))
        res = _run(c)
        assert not res["more"] and dr.stable(res["rows"], size, B, rk, R, cap, ml), seed
        assert res["moves"] >= res["rounds"] and res["proposals"] >= res["moves"], seed
        assert len(res["ssq"]) == res["rounds"] + 1 and all(y < x for x, y in zip(res["ssq"], res["ssq"][1:])), seed
        assert all(y <= x for x, y in zip(res["peaks"], res["peaks"][1:])), seed
        assert dr.rack_rule_holds(rows, res["rows"], rk, R, cap), seed
        assert ((res["rows"] == NONE) == (rows == NONE)).all() and (ml or (res["rows"][:, 0] == rows[:, 0]).all()), seed
        assert all(len(set(r)) == len(r) for r in ([b for b in row if b != NONE] for row in res["rows"].tolist())), seed
        lb, _ = dr.lower_bound(rows, size, B, ml)
        opt = dr.optimum(rows, size, B, rk, R, cap, ml)
        assert lb <= opt <= res["peak_after"] <= res["peak_before"], (seed, lb, opt, res["peak_after"], res["peak_before"])
        assert res["peak_after"] == int(dr.loads(res["rows"], size, B).max()) and int(dr.loads(res["rows"], size, B).sum()) == int(dr.loads(rows, size, B).sum())
        at_opt += res["peak_after"] == opt
        lb_at_opt += lb == opt
        proven += res["peak_after"] == lb
        moved += res["n_moved"] > 0
        padded += bool((rows == NONE).any())
        kept += not ml
        capped += cap > 0
        zeros += bool((size == 0).any())
    print(f"seeds={len(SEEDS)} peak==optimum: {at_opt}  lower_bound==optimum: {lb_at_opt}  proven: {proven}  moved: {moved}")
    assert moved >= 60 and padded >= 60 and kept == 60 and capped == 80 and zeros >= 60   # conditions on the inputs


def test_restatement_on_the_contention_shapes_and_limits():
    for B in (4, 5, 9):
        c = dr.crowded_case(B, 64)
        res = _run(c)
        S = dr.loads(res["rows"], c["size"], B)
        assert res["peak_before"] == 64 * 5 and res["peak_after"] - int(S.min()) <= 5, B   # equal sizes: stable means within one size
        assert dr.stable(res["rows"], c["size"], B, c["rack_of"], 1)
        one = _run(c, max_rounds=1)
        assert one["rounds"] == 1 and one["more"] and 1 <= one["moves"] <= min(3, B - 3)   # three sources, B - 3 destinations
        none = _run(c, min_gain=64 * 5)
        assert none["rounds"] == 0 and none["n_moved"] == 0 and (none["rows"] == c["rows"]).all() and not none["more"]
        kept = _run(c, move_leaders=False)
        assert (kept["rows"][:, 0] == c["rows"][:, 0]).all() and kept["n_moved"] > 0


def test_restatement_keeps_the_rack_rule():
    """One replica per rack and cap 1: every move stays inside its rack.  One rack, cap 1, width 3: the rows start over the cap and
    the moves are same-rack moves.  A row that holds every broker never moves."""
    rng = np.random.default_rng(3)
    B, R, P = 12, 3, 40
    rack_of = np.arange(B) % R
    rows = np.stack([rng.permutation(R) + R * rng.integers(0, 2, R) for _ in range(P)]).astype(np.int64)   # brokers 0..5 only, one per rack
    size = rng.integers(1, 100, P)
    res = dr.descend(rows, size, B, rack_of, R, cap=1)
    assert res["n_moved"] > 0 and (rack_of[res["rows"]] == rack_of[rows]).all()
    one = dr.descend(rows, size, B, np.zeros(B, dtype=np.int64), 1, cap=1)
    free = dr.descend(rows, size, B, np.zeros(B, dtype=np.int64), 1, cap=0)
    assert one["n_moved"] > 0 and one["rows"].tolist() == free["rows"].tolist()
    full = np.array([[2, 0, 1, 3], [0, 1, NONE, NONE], [0, 2, NONE, NONE]])
    res = dr.descend(full, [50, 1, 1], 4, np.zeros(4, dtype=np.int64), 1)
    assert res["rows"][0].tolist() == [2, 0, 1, 3]


def test_lower_bound_terms():
    rows = np.array([[0, 1], [0, 2], [0, NONE]])
    assert dr.lower_bound(rows, [4, 4, 4], 3, True) == (7, 1)      # ceil(20 / 3)
    assert dr.lower_bound(rows, [4, 4, 4], 3, False) == (12, 2)    # broker 0 leads all three
    assert dr.lower_bound(rows, [9, 1, 1], 3, True) == (9, 0)
    assert dr.lower_bound(rows, [0, 0, 0], 3, False) == (0, 0)     # the lowest term on ties
    assert dr.lower_bound(np.zeros((0, 2)), [], 3) == (0, 0)


def test_python_front_end_checks_its_arguments():
    from kafka_assignment_optimizer_amd.disk import balance_disk, balance_disk_arrays, sizes_of
    with pytest.raises(ValueError, match="rows"):
        balance_disk_arrays(np.zeros(4), 3, [0, 0, 0], 1, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="one value per row"):
        balance_disk_arrays(np.zeros((2, 2)), 3, [0, 0, 0], 1, [1])
    with pytest.raises(ValueError, match="one rack per broker"):
        balance_disk_arrays(np.array([[0, 1], [1, 2]]), 3, [0, 0], 1, [1, 2])
    with pytest.raises(ValueError, match=">= 0"):
        balance_disk_arrays(np.array([[0, 1], [1, 2]]), 3, [0, 0, 0], 1, [1, -1])
    with pytest.raises(ValueError, match="min_gain"):
        balance_disk_arrays(np.array([[0, 1], [1, 2]]), 3, [0, 0, 0], 1, [1, 2], min_gain=-1)
    keys = [("a", 0), ("a", 1), ("b", 7)]
    assert sizes_of(keys, {("a", 1): 5}, 9).tolist() == [9, 5, 9]
    with pytest.raises(ValueError, match="no size for partitions a-0, b-7 "):
        sizes_of(keys, {("a", 1): 5})
    doc = {"version": 1, "partitions": [{"topic": "a", "partition": 0, "replicas": [0, 1]}]}
    with pytest.raises(ValueError, match="no size for partitions a-0"):
        balance_disk(doc, {}, broker_list=[0, 1, 2], racks={0: "x", 1: "y", 2: "x"})
    with pytest.raises(ValueError, match="outside --broker-list"):
        balance_disk(doc, {("a", 0): 1}, broker_list=[0, 2], racks={0: "x", 2: "x"})
