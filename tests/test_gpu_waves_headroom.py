"""kao_plan_waves_headroom on the MI355X: waves as a sequence of states, each of which fits every disk.  Every
result is bit for bit the sequential reference of tests/waves_headroom_ref.py (wave, n_waves, lower_bound, stats[0..3] and [5..7])
and passes its independent checker; at capacity 2^63 it is also what kao_plan_waves_sized returns on the device.
One case per kernel path (wide broker indices, ties, capacities above 2^63, batch edges): tests/test_gpu_waves_headroom_paths.py."""
import numpy as np
import pytest

import waves_headroom_ref as hr
import waves_sized_ref as sr
from headroom_cases import HAND, hand_case

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
FACTORS = (100, 102, 110, 130)


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _exact(cur, tgt, size, stored, capacity, C, k, seed=1):
    """Runs the call, compares it with the reference and the checker; returns (wave, n_waves, lower_bound, stats)."""
    from kafka_assignment_optimizer_amd.waves import plan_waves_headroom_arrays
    B = len(stored)
    wave, nw, lb, stats = plan_waves_headroom_arrays(cur, tgt, B, size, stored, capacity, C, k, seed)
    mw, mnw, mlb, ms = hr.model(cur, tgt, size, stored, capacity, C, k, seed)
    assert (wave.tolist(), nw, lb) == (mw.tolist(), mnw, mlb)
    assert stats[:4].tolist() == ms[:4] and stats[5:].tolist() == ms[5:], (stats.tolist(), ms)
    assert hr.check_headroom(cur, tgt, size, stored, capacity, C, k, wave, nw, lb) == stats[0]
    assert stats[4] >= 1 or ms[2] < 0
    return wave, nw, lb, stats


def _instance(s):
    cur, tgt, size, C, k = sr.random_sized_instance(s)
    return cur, tgt, size, C, k, int(max(cur.max(), tgt.max())) + 1


@pytest.mark.parametrize("factor", FACTORS)
def test_random_instances_at_a_capacity_factor(kao, factor):
    for s in range(24):
        cur, tgt, size, C, k, B = _instance(s)
        st, cap = hr.scaled_capacity(cur, tgt, size, B, factor)
        _exact(cur, tgt, size, st, cap, C, k, seed=s + 1)


def test_unlimited_capacity_equals_the_sized_planner_on_the_device(kao):
    from kafka_assignment_optimizer_amd.waves import plan_waves_sized_arrays
    for s in range(24):
        cur, tgt, size, C, k, B = _instance(s)
        st = hr.stored_from_rows(cur, size, B)
        wave, nw, lb, stats = _exact(cur, tgt, size, st, [hr.UNLIMITED] * B, C, k, seed=s + 1)
        sw, snw, slb = plan_waves_sized_arrays(cur, tgt, B, size, C, k, s + 1)
        assert (wave.tolist(), nw, lb) == (sw.tolist(), snw, slb), s
        assert stats[0] == 0 and stats[1] == 0


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(kao, name):
    cur, tgt, size, st, cap, C, k = hand_case(name)
    want = HAND[name]["want"]
    wave, nw, _, stats = _exact(cur, tgt, size, st, cap, C, k)
    assert wave.tolist() == want["wave"] and nw == want["n_waves"]
    assert stats[1] == want.get("stuck_bytes", 0) and tuple(stats[5:].tolist()) == want["min_free"]


def test_width_1_width_8_padding_and_a_decommissioned_source(kao):
    # width 1: a ring of moves over 6 brokers with room for one arrival each
    cur = np.arange(6, dtype=np.uint16).reshape(6, 1)
    tgt = ((np.arange(6) + 1) % 6).astype(np.uint16).reshape(6, 1)
    size = np.array([10, 20, 30, 40, 50, 60], dtype=np.uint64)
    _exact(cur, tgt, size, [10, 20, 30, 40, 50, 60], [70] * 6, 0, 0)
    # width 8, rows padded with NONE; broker 11 is decommissioned: a source outside every target row
    cur = np.full((5, 8), NONE, dtype=np.uint16)
    tgt = np.full((5, 8), NONE, dtype=np.uint16)
    cur[0, :8] = [11, 1, 2, 3, 4, 5, 6, 7]
    tgt[0, :8] = [0, 1, 2, 3, 4, 5, 6, 8]
    cur[1, :3] = [11, 2, 3]
    tgt[1, :3] = [9, 2, 3]
    cur[2, :2] = [4, 11]
    tgt[2, :4] = [4, 0, 9, 10]
    cur[3, :3] = [5, 6, 7]
    tgt[3, :2] = [6, 5]                   # metadata-only: drops broker 7
    cur[4, :8] = [0, 1, 2, 3, 4, 5, 6, 7]
    tgt[4, :8] = [8, 9, 10, 3, 4, 5, 6, 7]
    size = np.array([100, 70, 30, 40, 25], dtype=np.uint64)
    st = hr.stored_from_rows(cur, size, 12)
    for cap in ([400] * 12, [200] * 12, [160] * 12):
        cap = [max(c, s) for c, s in zip(cap, st)]
        _exact(cur, tgt, size, st, cap, 0, 0)
        _exact(cur, tgt, size, st, cap, 150, 2)


def test_300_moving_partitions_on_20_brokers(kao):
    """More than one workgroup per order, and a ragged last wavefront (300 = 256 + 44)."""
    rng = np.random.default_rng(7)
    cur = np.array([rng.choice(20, 3, replace=False) for _ in range(300)], dtype=np.uint16)
    tgt = cur.copy()
    for p in range(300):
        free = [b for b in range(20) if b not in cur[p]]
        tgt[p, rng.integers(0, 3)] = rng.choice(free)
    size = rng.integers(1, 1000, 300).astype(np.uint64)
    st, cap = hr.scaled_capacity(cur, tgt, size, 20, 105)
    wave, nw, _, stats = _exact(cur, tgt, size, st, cap, 0, 4)
    assert (wave >= 0).sum() > 0
    _exact(cur, tgt, size, st, [hr.UNLIMITED] * 20, 3000, 0)


def test_70_waves_at_one_broker(kao):
    """Broker 0 receives 70 partitions at k = 1: 70 waves and more rounds than one batch, so the host loop iterates; the orders
    close their waves at different times."""
    cur = (np.arange(70, dtype=np.uint16) % 9 + 1).reshape(70, 1)
    tgt = np.zeros((70, 1), dtype=np.uint16)
    size = (np.arange(70, dtype=np.uint64) % 7 + 1)
    st = hr.stored_from_rows(cur, size, 10)
    wave, nw, lb, stats = _exact(cur, tgt, size, st, [1 << 20] * 10, 0, 1)
    assert nw == lb == 70 and sorted(wave.tolist()) == list(range(70)) and stats[4] > 32
    # the same with room for 100 bytes at broker 0: the waves end when it is full
    wave, nw, lb, stats = _exact(cur, tgt, size, st, [100] + [1 << 20] * 9, 0, 1)
    assert stats[0] > 0 and nw < 70


def test_sizes_above_2_32_and_near_2_61(kao):
    cur = np.array([[0, 1], [2, 3], [4, 5], [1, 0]], dtype=np.uint16)
    tgt = np.array([[0, 6], [6, 3], [4, 7], [1, 7]], dtype=np.uint16)
    big = (1 << 61) - 5
    size = np.array([big, (1 << 33) + 1, 1 << 40, 3], dtype=np.uint64)
    st = hr.stored_from_rows(cur, size, 8)
    st[6] = (1 << 61) + 9
    cap = [1 << 63] * 8
    cap[6] = st[6] + big + (1 << 33)        # room for the large arrival, one byte short of both
    cap[7] = (1 << 40) + 2                  # the 2^40 partition, one byte short of the 3 more
    wave, nw, _, stats = _exact(cur, tgt, size, st, cap, 0, 0)
    assert stats[0] == 2 and wave.tolist() == [0, -2, 0, -2] and stats[1] == (1 << 33) + 1 + 3
    cap[6] += 1
    cap[7] += 1
    assert _exact(cur, tgt, size, st, cap, 0, 0)[3][0] == 0


def test_no_caps_at_all(kao):
    for s in (1, 4, 11):
        cur, tgt, size, _, _, B = _instance(s)
        st, cap = hr.scaled_capacity(cur, tgt, size, B, 110)
        _, _, lb, _ = _exact(cur, tgt, size, st, cap, 0, 0, seed=3)
        assert lb == 1
        wave, nw, lb, _ = _exact(cur, tgt, size, st, [hr.UNLIMITED] * B, 0, 0)
        assert nw == lb == 1 and set(wave.tolist()) <= {-1, 0}


def test_stats_may_be_null_and_nothing_moves(kao):
    from kafka_assignment_optimizer_amd.waves import plan_waves_headroom_arrays
    cur, tgt, size, C, k, B = _instance(5)
    st, cap = hr.scaled_capacity(cur, tgt, size, B, 102)
    a = plan_waves_headroom_arrays(cur, tgt, B, size, st, cap, C, k, 9)
    b = plan_waves_headroom_arrays(cur, tgt, B, size, st, cap, C, k, 9, with_stats=False)
    assert b[3] is None and (a[0].tolist(), a[1], a[2]) == (b[0].tolist(), b[1], b[2])
    # nothing moves: a leader change only, and no partition at all
    cur = np.array([[0, 1], [1, 2]], dtype=np.uint16)
    wave, nw, lb, stats = _exact(cur, cur[:, ::-1].copy(), np.array([5, 5], dtype=np.uint64), [5, 10, 5], [10, 10, 10], 0, 0)
    assert (wave.tolist(), nw, lb, stats.tolist()) == ([0, 0], 1, 1, [0, 0, -1, 0, 0, -1, -1, -1])
    wave, nw, lb, stats = plan_waves_headroom_arrays(np.zeros((0, 2)), np.zeros((0, 2)), 3, np.zeros(0), [0] * 3, [0] * 3)
    assert (len(wave), nw, lb, stats.tolist()) == (0, 0, 0, [0, 0, -1, 0, 0, -1, -1, -1])


def test_the_same_call_twice_gives_the_same_answer(kao):
    from kafka_assignment_optimizer_amd.waves import plan_waves_headroom_arrays
    cur, tgt, size, C, k, B = _instance(17)
    st, cap = hr.scaled_capacity(cur, tgt, size, B, 100)
    a = plan_waves_headroom_arrays(cur, tgt, B, size, st, cap, C, k, 5)
    b = plan_waves_headroom_arrays(cur, tgt, B, size, st, cap, C, k, 5)
    assert a[0].tolist() == b[0].tolist() and a[1:3] == b[1:3] and a[3].tolist() == b[3].tolist()
