"""kao_balance_logdirs_capacity and kao_place_logdirs_capacity on the MI355X: the log-dir planners by utilisation L(d) / cap(d), one
workgroup per broker.  Every instance is held byte for byte (dir[], every number, per_broker, stats except
the launches) against the restatement in tests/logdirs_cap_ref.py; each runs twice for determinism and once with dry_run, and is
checked without the restatement: the peaks from recomputed loads by products, no replica off its broker, every homeless replica
placed, bound <= peak_after <= peak_before (balance), the proof column against the fractions, and the end state move-stable by
brute force."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import logdirs_cap_ref as cr
import logdirs_ref as lr
import place_ref as pr
from conftest import ROOT

pytestmark = pytest.mark.gpu

CUTOFF = 4096   # kLdSortLds of kao_logdirs.hip
BRUTE = 3000    # replicas up to which the brute-force stability check runs


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def balance(kao):
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays
    return balance_logdirs_arrays


@pytest.fixture(scope="module")
def place(kao):
    from kafka_assignment_optimizer_amd.logdirs import place_logdirs_arrays
    return place_logdirs_arrays


@contextlib.contextmanager
def sort_path(path):
    """The sort of this thread's calls (kao_logdirs_test_sort), put back on the way out."""
    from kafka_assignment_optimizer_amd import _ffi
    was = _ffi.load().kao_logdirs_test_sort(path)
    assert was >= 0
    try:
        yield
    finally:
        _ffi.load().kao_logdirs_test_sort(was)


def _u64(x):
    return None if x is None else np.asarray([int(v) for v in np.asarray(x, dtype=object).reshape(-1)], dtype=np.uint64)


def _rows(res):
    return [[int(x) for x in row] for row in res.per_broker]


def _fullest(L, cap):
    """{L, cap} of the fullest dir, ties to the lowest index; [0, 1] without dirs."""
    return list(cr.frac_max(list(zip(L, cap)))) if len(L) else [0, 1]


def _same(x, y, keys):
    return (x.dir.tobytes() == y.dir.tobytes() and all(getattr(x, k) == getattr(y, k) for k in keys) and x.per_broker.tobytes() == y.per_broker.tobytes()
            and x.stats.tolist() == y.stats.tolist())


B_KEYS = ("status", "n_moved", "bytes_moved", "peak_before_frac", "peak_after_frac")
P_KEYS = ("status", "n_placed", "bytes_placed", "n_moved", "bytes_moved", "peak_before_frac", "peak_after_frac")


def _checked_balance(balance, c, min_gain=0, max_rounds=0):
    """One instance through kao_balance_logdirs_capacity against the restatement; twice, once with dry_run; the invariants."""
    ds, d, w, cap, bs = c["dir_start"], np.asarray(c["dir"], dtype=np.int64), _u64(c["size"]), _u64(c["cap"]), _u64(c.get("base"))
    kw = dict(base=bs, min_gain=min_gain, max_rounds=max_rounds, capacity=cap)
    ref = cr.descend(ds, d, w, cap, bs, min_gain, max_rounds)
    res, again = (balance(ds, d, w, **kw) for _ in range(2))
    dry = balance(ds, d, w, dry_run=True, **kw)
    print(f"B={len(ds) - 1} D={int(np.asarray(ds)[-1])} R={len(d)} gpu={[getattr(res, k) for k in B_KEYS]} stats={res.stats.tolist()} ref={ref['stats']}")
    assert res.dir.astype(np.int64).tobytes() == ref["dir"].tobytes()
    assert (res.status, res.n_moved, res.bytes_moved) == (ref["status"], ref["n_moved"], ref["bytes_moved"])
    assert list(res.peak_before_frac) == ref["peak_before"] and list(res.peak_after_frac) == ref["peak_after"]
    assert (res.peak_before, res.peak_after) == (ref["peak_before"][0], ref["peak_after"][0])
    assert _rows(res) == ref["per_broker"]
    assert res.stats[:4].tolist() == ref["stats"][:4] and res.stats[5:].tolist() == ref["stats"][5:] and res.stats[4] in (2, 4)
    # without the restatement
    out, capl = res.dir.astype(np.int64), [int(x) for x in cap]
    L0, L1 = cr.loads(ds, d, w, bs), cr.loads(ds, out, w, bs)
    assert list(res.peak_before_frac) == _fullest(L0, capl) and list(res.peak_after_frac) == _fullest(L1, capl) and sum(L0) == sum(L1)
    assert (lr.broker_of_dir(ds)[out] == lr.broker_of_dir(ds)[d]).all() if len(d) else True
    moved = out != d
    assert (res.n_moved, res.bytes_moved) == (int(moved.sum()), sum(int(x) for x in w[moved]))
    for p in _rows(res):
        assert not cr.above(p[2], p[3], p[0], p[1]) and not cr.above(p[4], p[5], p[2], p[3])          # bound <= after <= before
        assert (p[9] == 1) == (p[2] * p[5] == p[4] * p[3]) and p[9] in (0, 1, 2)
    assert res.status == ("OPTIMAL_PROVEN" if all(p[9] for p in _rows(res)) else "FEASIBLE_BOUND_GAP") and res.stats[6] == sum(p[9] > 0 for p in _rows(res))
    if res.stats[5] == 0 and len(d) <= BRUTE:
        assert cr.stable_cap(ds, out, w, cap, bs, min_gain)
    assert _same(res, again, B_KEYS)
    assert (dry.dir == d).all() and dry.per_broker.tobytes() == res.per_broker.tobytes()
    assert all(getattr(dry, k) == getattr(res, k) for k in B_KEYS) and dry.stats.tolist() == res.stats.tolist()
    return res, ref


def _checked_place(place, c, move=False, min_gain=0, max_rounds=0, paths=False):
    """One instance through kao_place_logdirs_capacity against the restatement; twice, once with dry_run; the invariants; paths:
    through both sorts as well."""
    ds, br, d = c["dir_start"], np.asarray(c["broker"], dtype=np.int64), np.asarray(c["dir"], dtype=np.int64)
    w, cap, bs = _u64(c["size"]), _u64(c["cap"]), _u64(c.get("base"))
    kw = dict(base=bs, move_residents=move, min_gain=min_gain, max_rounds=max_rounds, capacity=cap)
    ref = cr.place(ds, br, d, w, cap, bs, move, min_gain, max_rounds)
    res, again = (place(ds, br, d, w, **kw) for _ in range(2))
    dry = place(ds, br, d, w, dry_run=True, **kw)
    print(f"B={len(ds) - 1} D={int(np.asarray(ds)[-1])} R={len(d)} move={move} gpu={[getattr(res, k) for k in P_KEYS]} stats={res.stats.tolist()} ref={ref['stats']}")
    assert res.dir.astype(np.int64).tobytes() == ref["dir"].tobytes()
    assert (res.status, res.n_placed, res.bytes_placed, res.n_moved, res.bytes_moved) == tuple(ref[k] for k in ("status", "n_placed", "bytes_placed", "n_moved", "bytes_moved"))
    assert list(res.peak_before_frac) == ref["peak_before"] and list(res.peak_after_frac) == ref["peak_after"]
    assert _rows(res) == ref["per_broker"]
    assert res.stats[:5].tolist() == ref["stats"][:5] and res.stats[6:].tolist() == ref["stats"][6:] and res.stats[5] in (2, 4)
    # without the restatement
    out, home, capl = res.dir.astype(np.int64), d < 0, [int(x) for x in cap]
    assert (out >= 0).all() and (res.n_placed, res.bytes_placed) == (int(home.sum()), sum(int(x) for x in w[home]))
    assert (lr.broker_of_dir(ds)[out] == br).all() if len(d) else True
    L0, L1 = cr.loads(ds, d, w, bs), cr.loads(ds, out, w, bs)
    assert list(res.peak_before_frac) == _fullest(L0, capl) and list(res.peak_after_frac) == _fullest(L1, capl)
    assert sum(L0) + sum(int(x) for x in w[home]) == sum(L1)
    moved = ~home & (out != d)
    assert (res.n_moved, res.bytes_moved) == (int(moved.sum()), sum(int(x) for x in w[moved])) and (move or not moved.any())
    for p in _rows(res):
        assert not cr.above(p[4], p[5], p[2], p[3]) and (p[11] == 1) == (p[2] * p[5] == p[4] * p[3]) and p[11] in (0, 1, 2)
    assert res.status == ("OPTIMAL_PROVEN" if all(p[11] for p in _rows(res)) else "FEASIBLE_BOUND_GAP")
    if len(d) <= BRUTE:
        if not move:
            assert cr.stable_cap(ds, out, w, cap, bs, only=[r for r in range(len(d)) if home[r]])
        elif res.stats[6] == 0:
            assert cr.stable_cap(ds, out, w, cap, bs, min_gain)
    assert _same(res, again, P_KEYS)
    assert (dry.dir == d).all() and dry.per_broker.tobytes() == res.per_broker.tobytes() and dry.stats.tolist() == res.stats.tolist()
    assert all(getattr(dry, k) == getattr(res, k) for k in P_KEYS)
    if paths:
        for path in (1, 2):
            with sort_path(path):
                assert _same(place(ds, br, d, w, **kw), res, P_KEYS)
    return res, ref


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_balance(balance):
    moved = kinds = 0
    for seed in range(120):
        res, _ = _checked_balance(balance, cr.small_case_cap(seed))
        moved += res.n_moved > 0
        kinds += len({p[9] for p in _rows(res)}) > 1
    print(f"calls with a move: {moved} of 120, with more than one kind of proof: {kinds}")
    assert moved >= 60


@pytest.mark.parametrize("move", [False, True])
def test_small_family_place(place, move):
    placed = 0
    for seed in range(120):
        res, _ = _checked_place(place, cr.small_place_case_cap(seed), move, paths=seed % 4 == 0)
        placed += res.n_placed > 0
    assert placed >= 90


# ---- 2. equal capacities are the byte planners -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1, 12345, None])
def test_equal_capacities_match_the_byte_entry_points(balance, place, value):
    """dir[], the counters, the bytes of the peaks, status, the L, moved, bytes, placed and rounds columns, every stats entry but the
    launch count; None: 2^61 / n_dirs."""
    for seed in range(0, 120, 2):
        c = lr.small_case(seed)
        D = int(c["dir_start"][-1])
        cap = np.full(D, 2 ** 61 // max(D, 1) if value is None else value, dtype=np.uint64)
        x, y = balance(c["dir_start"], c["dir"], c["size"], c["base"], capacity=cap), balance(c["dir_start"], c["dir"], c["size"], c["base"])
        assert x.dir.tobytes() == y.dir.tobytes() and (x.status, x.n_moved, x.bytes_moved, x.peak_before, x.peak_after) == (y.status, y.n_moved, y.bytes_moved, y.peak_before, y.peak_after)
        assert x.per_broker[:, [0, 2, 6, 7, 8]].tolist() == y.per_broker[:, [0, 1, 3, 4, 5]].tolist()
        assert np.delete(x.stats, 4).tolist() == np.delete(y.stats, 4).tolist()
        c = pr.small_case(seed)
        for move in (False, True):
            x = place(c["dir_start"], c["broker"], c["dir"], c["size"], c["base"], move, capacity=cap)
            y = place(c["dir_start"], c["broker"], c["dir"], c["size"], c["base"], move)
            assert x.dir.tobytes() == y.dir.tobytes() and np.delete(x.stats, 5).tolist() == np.delete(y.stats, 5).tolist()
            assert (x.status, x.n_placed, x.bytes_placed, x.n_moved, x.bytes_moved, x.peak_before, x.peak_after) == (y.status, y.n_placed, y.bytes_placed, y.n_moved, y.bytes_moved, y.peak_before, y.peak_after)
            assert x.per_broker[:, [0, 2, 6, 7, 8, 9, 10]].tolist() == y.per_broker[:, [0, 1, 3, 4, 5, 6, 7]].tolist()


def test_place_without_homeless_is_the_balance_call(balance, place):
    for seed in range(0, 120, 3):
        c = cr.small_case_cap(seed)
        broker = lr.broker_of_dir(c["dir_start"])[c["dir"]] if len(c["dir"]) else np.zeros(0, dtype=np.int64)
        x = place(c["dir_start"], broker, c["dir"], c["size"], c["base"], True, capacity=c["cap"])
        y = balance(c["dir_start"], c["dir"], c["size"], c["base"], capacity=c["cap"])
        assert x.dir.tobytes() == y.dir.tobytes() and (x.status, x.n_moved, x.bytes_moved, x.peak_before_frac, x.peak_after_frac) == (y.status, y.n_moved, y.bytes_moved, y.peak_before_frac, y.peak_after_frac)
        assert x.per_broker[:, [0, 1, 2, 3, 4, 5, 8, 9, 10, 11]].tolist() == y.per_broker.tolist() and x.n_placed == 0


# ---- 3. dir counts and bucket sizes ------------------------------------------------------------------------------------------------------
def _unequal_caps(rng, D):
    """Every fourth dir a quarter of the others, each a little off so that no two utilisations tie by accident."""
    return np.where(np.arange(D) % 4 == 0, 2 ** 28, 2 ** 30) + rng.integers(0, 1000, D)


def test_dir_counts_0_1_2_63_64_in_one_call(balance, place):
    rng = np.random.default_rng(11)
    nd = [0, 1, 2, 63, 64, 0, 3]
    ds = np.concatenate([[0], np.cumsum(nd)])
    dirs, brokers = [], []
    for b, n in enumerate(nd):
        if n:
            k = 2 * n + 5
            dirs.append(ds[b] + (rng.random(k) ** 3 * n).astype(np.int64))   # skewed toward the low dirs
            brokers.append(np.full(k, b))
    d, br = np.concatenate(dirs), np.concatenate(brokers)
    perm = rng.permutation(len(d))
    d, br = d[perm], br[perm]
    size = rng.integers(0, 2 ** 24, len(d))
    c = dict(dir_start=ds, dir=d, size=size, base=rng.integers(0, 2 ** 22, int(ds[-1])), cap=_unequal_caps(rng, int(ds[-1])))
    res, _ = _checked_balance(balance, c)
    assert res.per_broker[0].tolist() == [0, 1, 0, 1, 0, 1, 0, 0, 0, 1] and res.per_broker[1, 6] == 0 and res.per_broker[4, 6] > 0
    home = d.copy()
    home[rng.random(len(d)) < 0.4] = -1
    for move in (False, True):
        res, _ = _checked_place(place, dict(c, broker=br, dir=home), move, paths=True)
        assert res.per_broker[5].tolist() == [0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1]


@pytest.mark.parametrize("n", [255, 256, 257, 1024, 1025])
def test_bucket_sizes_around_the_lane_switch(balance, place, n):
    """The largest bucket decides between 256 and 1,024 lanes a workgroup."""
    rng = np.random.default_rng(n)
    c = lr.lognormal_case(1, 5, n, 0.8, n, based=0.4)
    small = lr.lognormal_case(2, 3, 20, 0.5, n + 1)
    ds = np.concatenate([c["dir_start"], 5 + small["dir_start"][1:]])
    d, size = np.concatenate([c["dir"], 5 + small["dir"]]), np.concatenate([c["size"], small["size"]])
    perm = rng.permutation(len(d))
    case = dict(dir_start=ds, dir=d[perm], size=size[perm], base=np.concatenate([c["base"], small["base"]]), cap=_unequal_caps(rng, 11))
    res, _ = _checked_balance(balance, case)
    assert res.n_moved > 0
    home = case["dir"].copy()
    home[rng.random(len(d)) < 0.3] = -1
    _checked_place(place, dict(case, broker=lr.broker_of_dir(ds)[case["dir"]], dir=home), True)


# ---- 4. the arithmetic ---------------------------------------------------------------------------------------------------------------
def test_capacity_1_beside_2_to_the_61(balance, place):
    """u = L / 1 beside u = L / 2^61: everything belongs on the large dir, whatever it already holds."""
    ds, cap = [0, 2, 4], [1, 2 ** 61, 2 ** 60, 1]
    c = dict(dir_start=ds, dir=[0, 0, 1, 0, 3, 3, 2], size=[5, 2 ** 40, 7, 0, 2 ** 50, 3, 9], base=[0, 2 ** 55, 0, 0], cap=cap)
    res, _ = _checked_balance(balance, c)
    assert res.dir.tolist() == [1, 1, 1, 0, 2, 2, 2] and res.status == "OPTIMAL_PROVEN"
    c = dict(c, broker=[0, 0, 0, 0, 1, 1, 1], dir=[-1, 0, -1, -1, 3, -1, 2])
    res, _ = _checked_place(place, c, False, paths=True)
    assert res.dir.tolist() == [1, 0, 1, 1, 3, 2, 2]
    _checked_place(place, c, True, paths=True)


def test_loads_near_2_to_the_61_products_pass_64_bits(balance, place):
    rng = np.random.default_rng(5)
    size = np.concatenate([[2 ** 60, 2 ** 59, 2 ** 59 + 12345], rng.integers(2 ** 50, 2 ** 54, 40)])
    c = dict(dir_start=[0, 4, 7], dir=np.concatenate([[0, 0, 0], rng.integers(0, 7, 40)]), size=size, base=[0, 0, 2 ** 59, 0, 0, 7, 0],
             cap=[2 ** 58, 2 ** 59, 2 ** 58 + 1, 2 ** 57 + 3, 3 * 2 ** 55, 2 ** 55, 2 ** 55 + 9])
    c["dir"][:3] = 0
    c["dir"][3:] = np.where(c["dir"][3:] < 4, 4, c["dir"][3:])   # the forty on broker 1; the three large ones on broker 0
    res, _ = _checked_balance(balance, c)
    assert res.n_moved > 0
    br = lr.broker_of_dir(c["dir_start"])[c["dir"]]
    home = c["dir"].copy()
    home[::3] = -1
    for move in (False, True):
        _checked_place(place, dict(c, broker=br, dir=home), move, paths=True)


def test_utilisations_that_agree_in_their_first_53_bits(balance, place):
    """A = (2^60 + 1) / 2^60 and B = (2^60 + 3) / (2^60 + 2) differ by about 2^-119: doubles hold both as the same number, the
    products say A > B.  The gain test: a replica of 5 bytes leaves a dir at A for one that it brings to B, and does not leave a dir
    at B for one that it would bring to A."""
    A, B = (2 ** 60 + 1, 2 ** 60), (2 ** 60 + 3, 2 ** 60 + 2)
    assert float(A[0]) / float(A[1]) == float(B[0]) / float(B[1]) and cr.above(*A, *B)
    res, _ = _checked_balance(balance, dict(dir_start=[0, 2], dir=[0], size=[5], base=[A[0] - 5, B[0] - 5], cap=[A[1], B[1]]))
    assert res.dir.tolist() == [1] and res.peak_after_frac == B
    res, _ = _checked_balance(balance, dict(dir_start=[0, 2], dir=[0], size=[5], base=[B[0] - 5, A[0] - 5], cap=[B[1], A[1]]))
    assert res.dir.tolist() == [0] and res.n_moved == 0
    # ranked by products: dir 1 is the fuller one although a double cannot tell
    c = dict(dir_start=[0, 3], dir=[0, 1, 1], size=[2, 2, 2 ** 30], base=[B[0] - 2, A[0] - 2 - 2 ** 30, 0], cap=[B[1], A[1], 2 ** 59])
    res, _ = _checked_balance(balance, c)
    assert res.per_broker[0, :2].tolist() == [A[0], A[1]] and res.n_moved >= 1
    # PLACE: 5 bytes onto the dir that is the least full WITH them: B, not A, wherever each one sits
    for caps, bases, want in (((A[1], B[1]), (A[0] - 5, B[0] - 5), 1), ((B[1], A[1]), (B[0] - 5, A[0] - 5), 0)):
        res, _ = _checked_place(place, dict(dir_start=[0, 2], broker=[0], dir=[-1], size=[5], base=list(bases), cap=list(caps)), False, paths=True)
        assert res.dir.tolist() == [want]


def test_min_gain_limits(balance, place):
    """min_gain = 2^64 - 1 and one that makes the 64-bit sum on the left overflow: no move passes; just below, moves pass."""
    c = cr.small_case_cap(7)
    big = dict(dir_start=[0, 3], dir=[0, 0, 0, 1], size=[2 ** 59, 2 ** 59, 2 ** 58, 5], base=[2 ** 60, 0, 0], cap=[2 ** 59, 2 ** 60, 2 ** 58])
    for case in (c, big):
        for mg in (2 ** 64 - 1, 2 ** 64 - 2 ** 59, 2 ** 63):
            res, _ = _checked_balance(balance, case, min_gain=mg)
            assert res.n_moved == 0 and res.stats[1] == 0
    res, _ = _checked_balance(balance, big, min_gain=2 ** 58)
    assert res.n_moved > 0
    pc = cr.small_place_case_cap(7)
    res, _ = _checked_place(place, pc, True, min_gain=2 ** 64 - 1)
    assert res.n_moved == 0 and res.n_placed > 0


def test_max_rounds_and_zero_sizes(balance, place):
    c = lr.lognormal_case(3, 6, 200, 0.9, 21, zeros=0.3)
    c["cap"] = _unequal_caps(np.random.default_rng(3), 18)
    free, _ = _checked_balance(balance, c)
    assert free.stats[7] > 2
    for k in (1, 2):
        res, _ = _checked_balance(balance, c, max_rounds=k)
        assert res.stats[7] == k and res.stats[5] == 3 and not cr.above(*free.peak_after_frac, *res.peak_after_frac)
    zero = dict(c, size=np.zeros_like(c["size"]))
    res, _ = _checked_balance(balance, zero)
    assert res.n_moved == 0 and res.peak_after == 0
    br = lr.broker_of_dir(c["dir_start"])[c["dir"]]
    res, _ = _checked_place(place, dict(zero, broker=br, dir=np.where(np.arange(600) % 2, -1, c["dir"])), True, paths=True)
    assert res.n_placed == 300 and res.bytes_placed == 0
    _checked_place(place, dict(c, broker=br, dir=np.where(np.arange(600) % 2, -1, c["dir"])), True, max_rounds=1)


def test_64_dirs_every_replica_on_dir_0(balance):
    rng = np.random.default_rng(64)
    c = lr.crowded_case(64, 240, base=100)
    c["cap"] = rng.integers(1000, 9000, 64)
    res, _ = _checked_balance(balance, c)
    assert res.n_moved > 200 and cr.above(*res.peak_before_frac, *res.peak_after_frac)
    used = np.bincount(res.dir, minlength=64)
    assert (used > 0).all() and used[np.argmax(c["cap"])] > used[np.argmin(c["cap"])]


# ---- 5. homeless counts ----------------------------------------------------------------------------------------------------------------
def _one_big(k, n, residents, seed):
    """Broker 1 has n dirs, `residents` residents and k homeless replicas; three small brokers around it; the array order is shuffled."""
    big = lr.lognormal_case(1, n, residents + k, 0.7, seed)
    rng = np.random.default_rng(seed)
    bd = big["dir"].copy()
    bd[rng.permutation(residents + k)[:k]] = -1
    ds = np.array([0, 2, 2 + n, 4 + n, 6 + n])
    d = np.concatenate([[0, -1], np.where(bd >= 0, bd + 2, -1), [2 + n, -1, 5 + n]])
    broker = np.concatenate([[0, 0], np.ones(residents + k, dtype=np.int64), [2, 2, 3]])
    size = np.concatenate([[700, 30], big["size"], [0, 55, 900]])
    perm = rng.permutation(len(d))
    return dict(dir_start=ds, broker=broker[perm], dir=d[perm], size=size[perm], base=None, cap=_unequal_caps(rng, 6 + n))


@pytest.mark.parametrize("move", [False, True])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, CUTOFF, CUTOFF + 1])
def test_homeless_counts(kao, place, k, move):
    """Below, at and above a chunk of the greedy pass and the two sides of the cut-off between the sorts; both sorts are forced
    wherever both can run, and the LDS sort refuses a count above the cut-off."""
    c = _one_big(k, 4, 40, 100 + k)
    res, _ = _checked_place(place, c, move, paths=k <= CUTOFF)
    assert res.per_broker[1, 6] == k and res.stats[9] == max(k, 1)
    if k > CUTOFF:
        with sort_path(1):
            with pytest.raises(kao.KaoError) as e:
                place(c["dir_start"], c["broker"], c["dir"], c["size"], capacity=c["cap"])
        assert e.value.code == -2 and "kao_place_logdirs_capacity: " in str(e.value)


# ---- 6. many brokers: every row is the restatement on that broker alone ------------------------------------------------------------------
def test_300_brokers_rows_equal_the_brokers_alone(balance, place):
    c = lr.lognormal_case(300, 4, 40, 0.8, 300, based=0.3)
    rng = np.random.default_rng(300)
    c["cap"] = _unequal_caps(rng, 1200)
    res = balance(c["dir_start"], c["dir"], c["size"], c["base"], capacity=c["cap"])
    br = lr.broker_of_dir(c["dir_start"])[c["dir"]]
    home = c["dir"].copy()
    home[rng.random(len(home)) < 0.5] = -1
    pc = dict(c, broker=br, dir=home)
    got = {m: place(c["dir_start"], br, home, c["size"], c["base"], m, capacity=c["cap"]) for m in (False, True)}
    fulls = [cr.frac_max([(int(r[2]), int(r[3])) for r in x.per_broker]) for x in (res, got[False], got[True])]
    assert [tuple(x.peak_after_frac) for x in (res, got[False], got[True])] == fulls
    for b in range(300):
        sub, mine = cr.one_broker(c, b)
        ref = cr.descend(sub["dir_start"], sub["dir"], sub["size"], sub["cap"], sub["base"], ids=mine)
        assert [int(x) for x in res.per_broker[b]] == ref["per_broker"][0] and (res.dir[mine] - 4 * b).tolist() == ref["dir"].tolist()
        sub, mine = cr.one_place_broker(pc, b)
        for m in (False, True):
            ref = cr.place(sub["dir_start"], sub["broker"], sub["dir"], sub["size"], sub["cap"], sub["base"], m, ids=mine)
            assert [int(x) for x in got[m].per_broker[b]] == ref["per_broker"][0] and (got[m].dir[mine] - 4 * b).tolist() == ref["dir"].tolist()
    assert res.stats[0] > 250 and got[True].stats[0] == 300


# ---- 7. the refusals hold with a device too ------------------------------------------------------------------------------------------------
def test_refusals_with_a_device():
    import test_logdirs_cap_errors as host
    for entry in ("balance", "place"):
        for what, change, code, text in host.REFUSED[entry]:
            rc, msg = host.CALLS[entry](**change)
            assert rc == code and text in msg, (entry, what)


# ---- 8. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-logdirs")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.logdirs"])


def _both(args, tmp_path, tag):
    """Each tool in a fresh child process: the same --out document and the same report."""
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"{tag}{i}.json"
        r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    return outs[0][0], outs[0][1].splitlines()


def test_cli_against_python(kao, tmp_path):
    """cli/kao-logdirs and the Python twin with --utilisation and with --capacities, in every mode: the same plan file and the same
    report, both the library's; the small volume ends no fuller than the byte plan leaves it."""
    import test_logdirs_cap_errors as host
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs, place_logdirs
    doc, logdirs, caps_by_dir, caps_by_broker = host.cluster_documents()
    paths = host.write_documents(tmp_path, doc, logdirs, caps_by_dir, caps_by_broker)
    base = ["--current", paths["current"], "--log-dirs", paths["logdirs"]]
    text = open(paths["logdirs"]).read()
    plan_doc = json.load(open(paths["plan"]))
    for tag, flags, kw in (("util", ["--utilisation", "--default-capacity", "24M"], dict(use_total_bytes=True, default_capacity=24 * 2 ** 20)),   # two dirs have no totalBytes
                           ("caps", ["--capacities", paths["caps_by_dir"]], dict(capacity=caps_by_dir)),
                           ("mixed", ["--capacities", paths["caps_by_broker"], "--utilisation", "--default-capacity", "3G"],
                            dict(capacity=caps_by_broker, use_total_bytes=True, default_capacity=3 * 2 ** 30))):
        out, report = _both(base + flags, tmp_path, tag)
        lib = balance_logdirs(doc, text, **kw)
        assert out.decode() == lib.text() and report == lib.report_lines() and lib.result.peak_after_frac is not None
        assert " peak_after_ppm=" in report[0] and " proof=" in report[0] and " peak_after_ppm=" in report[-1]
        assert lib.result.n_moved > 0
        for mode, margs, mkw in (("plan", ["--plan", paths["plan"]], dict(plan_doc=plan_doc)),
                                 ("evac", ["--evacuate", host.EVACUATE, "--rebalance"], dict(evacuate=[host.EVACUATE_PAIR], rebalance=True)),
                                 ("dry", ["--plan", paths["plan"], "--dry-run"], dict(plan_doc=plan_doc, dry_run=True))):
            out, report = _both(base + flags + margs, tmp_path, tag + mode)
            lib = place_logdirs(doc, text, **mkw, **kw)
            assert out.decode() == lib.text() and report == lib.report_lines() and " proof=" in report[0]
            assert lib.result.n_placed > 0
    byte_plan, cap_plan = balance_logdirs(doc, text), balance_logdirs(doc, text, use_total_bytes=True, default_capacity=24 * 2 ** 20)
    caps = cap_plan.capacity
    L_byte = cr.loads(cap_plan.input.dir_start, byte_plan.result.dir, cap_plan.input.size, cap_plan.input.base)
    assert not cr.above(*cap_plan.result.peak_after_frac, *cr.frac_max(list(zip(L_byte, [int(x) for x in caps]))))
