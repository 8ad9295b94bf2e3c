"""CPU tests of the reference of kao_plan_waves_headroom (tests/waves_headroom_ref.py): at unlimited capacity the sequential loop
is the sized planner's first fit; its plans pass the independent checker at four capacity factors, stuck or complete; hand cases
with hand-counted answers; and the exhaustive search on the small stuck plans (measured, not asserted)."""
import numpy as np
import pytest

import waves_headroom_ref as hr
import waves_sized_ref as sr
from headroom_cases import HAND, hand_case

FACTORS = (100, 102, 110, 130)   # capacity = floor(max(stored, final) * s / 100)


def _instance(s):
    cur, tgt, size, C, k = sr.random_sized_instance(s)
    return cur, tgt, size, C, k, int(max(cur.max(), tgt.max())) + 1


def test_unlimited_capacity_is_the_sized_first_fit():
    for s in range(200):
        cur, tgt, size, C, k, B = _instance(s)
        st = hr.stored_from_rows(cur, size, B)
        w, nw, lb, stats = hr.model(cur, tgt, size, st, [hr.UNLIMITED] * B, C, k, s + 1)
        mw, mnw, mlb, win = sr.kernel_model_sized(cur, tgt, size, C, k, s + 1, with_winner=True)
        assert (w.tolist(), nw, lb, stats[2]) == (mw.tolist(), mnw, mlb, win), s
        assert stats[0] == stats[1] == 0 and stats[3] == (64 if win >= 0 else 0)


@pytest.mark.parametrize("factor", FACTORS)
def test_checker_passes_at_every_capacity_factor(factor):
    """Both outcomes occur: plans stuck in every order (149 / 87 / 55 / 20 of the 200 seeds at the four factors) and complete ones."""
    stuck_plans = 0
    for s in range(200):
        cur, tgt, size, C, k, B = _instance(s)
        st, cap = hr.scaled_capacity(cur, tgt, size, B, factor)
        w, nw, lb, stats = hr.model(cur, tgt, size, st, cap, C, k, s + 1)
        assert hr.check_headroom(cur, tgt, size, st, cap, C, k, w, nw, lb) == stats[0], s
        stuck_plans += stats[0] > 0
    assert 0 < stuck_plans < 200
    assert stuck_plans == {100: 149, 102: 87, 110: 55, 130: 20}[factor]


def test_checker_refuses_an_overfull_wave_and_a_partition_that_is_not_stuck():
    cur, tgt, size, st, cap, C, k = hand_case("chain")
    w, nw, lb, _ = hr.model(cur, tgt, size, st, cap, C, k, 1)
    assert hr.check_headroom(cur, tgt, size, st, cap, C, k, w, nw, lb) == 0
    with pytest.raises(AssertionError):   # both in one wave: broker 1 would hold 100 + 60
        hr.check_headroom(cur, tgt, size, st, cap, C, k, [0, 0], 1, lb)
    with pytest.raises(AssertionError):   # the 1 -> 2 move called stuck although broker 2 is empty
        hr.check_headroom(cur, tgt, size, st, cap, C, k, [-2, -2], 0, lb)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    cur, tgt, size, st, cap, C, k = hand_case(name)
    want = HAND[name]["want"]
    w, nw, lb, stats = hr.model(cur, tgt, size, st, cap, C, k, 1)
    assert hr.check_headroom(cur, tgt, size, st, cap, C, k, w, nw, lb) == stats[0]
    assert w.tolist() == want["wave"] and nw == want["n_waves"], (w.tolist(), nw)
    assert stats[0] == want["wave"].count(-2) and stats[1] == want.get("stuck_bytes", 0)
    if "min_free" in want:
        assert tuple(stats[5:8]) == want["min_free"], stats[5:8]


def test_three_partition_case_needs_another_order():
    """Order 0 (all keys tie on traffic and degree, so by index: p first) gets stuck; the best of the orders completes."""
    cur, tgt, size, st, cap, C, k = hand_case("order_decides")
    cls, parts, traf = sr.traffic(cur, tgt, size)
    wv, nw, _ = hr.run_order(cls, parts, traf, hr.add_rem(cur, tgt), size, st, cap, C, k, sr.sized_order(parts, traf, 0, 1))
    assert sr.sized_order(parts, traf, 0, 1) == [0, 1, 2]
    assert [wv[p] for p in range(3)] == [0, -2, -2] and nw == 1
    w, nw, _, stats = hr.model(cur, tgt, size, st, cap, C, k, 1)
    assert stats[0] == 0 and nw == 3 and stats[2] > 0
    assert hr.can_complete(cur, tgt, size, st, cap) is True


def test_order_count_rule():
    assert hr.order_count(1000, 100000) == 64
    assert hr.order_count(65534, 0) == 64                      # 60 bytes per broker: 64 orders take 240 MiB
    assert hr.order_count(1000, 4 << 20) == (1 << 30) // (60000 + (4 << 20) * 8) == 31
    assert hr.order_count(65534, 1 << 28) == 1


def test_exhaustive_search_on_hand_cases():
    for name, complete in (("swap", False), ("chain", True), ("exact_fit_over", False), ("exact_fit", True)):
        cur, tgt, size, st, cap, _, _ = hand_case(name)
        assert hr.can_complete(cur, tgt, size, st, cap) is complete, name


def test_measured_stuck_plans_an_exhaustive_order_completes(capsys):
    """Measured, not asserted: of the plans stuck in every order with at most 14 moving partitions, how many
    some one-at-a-time order completes.  The figures are printed; only their consistency is checked."""
    for factor in (100, 102, 110):
        small = done = 0
        for s in range(200):
            cur, tgt, size, C, k, B = _instance(s)
            st, cap = hr.scaled_capacity(cur, tgt, size, B, factor)
            if hr.model(cur, tgt, size, st, cap, C, k, s + 1)[3][0] == 0:
                continue
            r = hr.can_complete(cur, tgt, size, st, cap)
            if r is not None:
                small += 1
                done += bool(r)
        with capsys.disabled():
            print(f"\nheadroom factor {factor / 100}: {done} of {small} small stuck plans have a completing order")
        assert 0 <= done <= small
