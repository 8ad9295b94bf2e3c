"""CPU tests of the disk-usage balance with exchange moves (kao_balance_disk_exchange): the restatement of the
two kinds of round in tests/disk_x_ref.py, which asserts in every round that the loads agree with the rows, the sum of S^2 falls, the
peak does not rise, winners share no broker and no partition, rows hold no broker twice and the rack rule holds, and on instances of
up to 100 partitions that a partition proposes iff some pair passes.  Here: the small family ends move-stable and exchange-stable
between the optimum and the plain call's peak, with the counts of section 4u pinned; equal sizes give the plain call's bytes; the
hand-built cases behave as their docstrings say; max_rounds stops where it should."""
import functools

import numpy as np
import pytest

import disk_ref as dr
import disk_x_ref as dx

NONE = 0xFFFF
SEEDS = range(120)


@pytest.fixture(autouse=True, scope="module")
def bound():
    """The reference restates an entry point: without it there is nothing to hold it against."""
    from kafka_assignment_optimizer_amd import _ffi
    assert "kao_balance_disk_exchange" in _ffi.SIGNATURES
    return _ffi.load().kao_balance_disk_exchange


def _plain(c, **kw):
    return dr.descend(c["rows"], c["size"], c["B"], c["rack_of"], c["R"], c.get("cap", 0), c.get("move_leaders", True), **kw)


@functools.lru_cache(maxsize=None)
def _mid():
    """One instance with both kinds of round interleaved (83 move rounds, then exchange rounds with three more bursts of moves): the
    case and its full run."""
    c = dict(dr.lognormal_case(10, 2, 200, 3, 0.7, 7), cap=0, move_leaders=True)
    return c, dx.run(c)


def test_small_family_ends_stable_between_the_optimum_and_the_plain_peak():
    """lower_bound <= optimum <= peak_after <= descend's peak at min_gain 0 and 5, the ends move-stable and exchange-stable by brute
    force; an exchange round only ever follows a state the plain call ends at, so stats[11] is its peak.  The counts at min_gain 0 are
    those of DESIGN.md section 4u."""
    at_opt = plain_at_opt = lower = x_rounds = exchanges = proven = shared = stable = 0
    for seed in SEEDS:
        c = dr.small_case(seed)
        rows, size, B, rk, R, cap, ml = (c[k] for k in ("rows", "size", "B", "rack_of", "R", "cap", "move_leaders"))
        lb, _ = dr.lower_bound(rows, size, B, ml)
        opt = dr.optimum(rows, size, B, rk, R, cap, ml)
        for mg in (0, 5):
            plain, res = _plain(c, min_gain=mg), dx.run(c, min_gain=mg)
            assert lb <= opt <= res["peak_after"] <= plain["peak_after"], (seed, mg)
            assert res["x_peak"] == plain["peak_after"] and not res["more"] and res["kinds"].startswith("m" * plain["rounds"]), (seed, mg)
            assert dr.stable(res["rows"], size, B, rk, R, cap, ml, mg) and dx.exchange_stable(res["rows"], size, B, rk, R, cap, ml, mg), (seed, mg)
            stable += 1
            assert res["rounds"] == len(res["kinds"]) and res["x_rounds"] == res["kinds"].count("x") and res["moves"] >= res["exchanges"] >= res["x_rounds"]
            assert (res["n_moved"], res["bytes_moved"]) == dr.set_moves(rows, res["rows"], size)
            if res["x_rounds"] == 0:
                assert res["rows"].tobytes() == plain["rows"].tobytes()
            if mg == 0:
                at_opt += res["peak_after"] == opt
                plain_at_opt += plain["peak_after"] == opt
                lower += res["peak_after"] < plain["peak_after"]
                x_rounds += res["x_rounds"]
                exchanges += res["exchanges"]
                shared += res["shared"]
                proven += res["peak_after"] == lb
    print(f"optimum reached: {plain_at_opt} -> {at_opt}  strictly lower: {lower}  exchange rounds: {x_rounds}  exchanges: {exchanges}  proven: {proven}  "
          f"rounds with a partition named by two broker-winners: {shared}  stable ends: {stable}")
    assert (plain_at_opt, at_opt, lower, x_rounds, exchanges, proven, shared, stable) == PINNED


PINNED = (65, 85, 49, 207, 253, 55, 9, 240)   # from the restatement itself; DESIGN.md section 4u carries the same numbers


def test_equal_sizes_get_the_plain_calls_bytes():
    """All positive sizes equal: delta > 0 never holds, so a move-stable state is exchange-stable."""
    seen = 0
    for seed in range(0, 120, 10):   # small_case gives these seeds one size, 7, with a tenth of them zero
        c = dr.small_case(seed)
        assert set(np.unique(c["size"]).tolist()) <= {0, 7}
        plain, res = _plain(c), dx.run(c)
        assert res["rows"].tobytes() == plain["rows"].tobytes() and res["exchanges"] == res["x_rounds"] == res["x_proposals"] == 0
        assert (res["rounds"], res["moves"], res["proposals"]) == (plain["rounds"], plain["moves"], plain["proposals"]) and res["x_peak"] == plain["peak_after"]
        seen += 1
    c = dr.crowded_case(5, 64)
    assert dx.run(c)["rows"].tobytes() == _plain(c)["rows"].tobytes()
    assert seen == 12


def test_a_partition_named_by_two_broker_winners_is_written_by_one():
    c = dx.shared_partner_case()
    one = dx.run(c, max_rounds=1)
    assert one["kinds"] == "x" and one["shared"] == 1 and one["x_proposals"] == 2 and one["exchanges"] == 1 and one["more"]
    assert one["rows"][2].tolist() == [4, 2, 0] and one["rows"][0].tolist() == [4, 3, NONE] and one["rows"][1].tolist() == [4, 1, 3]   # x1 won y, x2 waits
    full = dx.run(c)
    assert full["kinds"] == "xx" and full["exchanges"] == 2 and full["peak_after"] == full["x_peak"] == 26   # the parked leaders are the peak
    assert dx.exchange_stable(full["rows"], c["size"], c["B"], c["rack_of"], c["R"], 0, False)


def test_only_a_member_before_the_split_passes_when_min_gain_is_half_the_gap():
    c = dx.narrow_gain_case()
    tight = dx.run(c, min_gain=5)
    assert tight["kinds"] == "x" and tight["rows"].tolist() == [[2, 1], [2, 0], [2, 1], [2, 1], [0, NONE]]   # y8: delta 2, 2 + 5 < 8
    loose = dx.run(c)
    assert loose["kinds"] == "x" and loose["rows"].tolist() == [[2, 1], [2, 1], [2, 1], [2, 0], [0, NONE]]   # y6: |2 * 4 - 8| = 0
    assert dx.run(c, min_gain=7)["kinds"] == ""   # delta + 7 < 8 needs delta < 1
    assert dx.run(c, min_gain=2 ** 64 - 1)["kinds"] == "" and dx.run(c, min_gain=2 ** 62)["x_peak"] == 31


def test_rack_rule_refuses_the_partner_and_a_lighter_one_is_taken():
    c = dx.rack_partner_case()
    capped = dx.run(c)
    assert capped["kinds"] == "x" and capped["rows"].tolist() == [[2, 1], [2, 1], [3, 0], [0, NONE], [3, NONE]]   # yB
    free = dx.run(c, cap=0)
    assert free["kinds"] == "x" and free["rows"].tolist() == [[2, 1], [2, 0], [3, 1], [0, NONE], [3, NONE]]       # yA
    assert dr.rack_rule_holds(c["rows"], capped["rows"], c["rack_of"], c["R"], 1) and not dr.rack_rule_holds(c["rows"], free["rows"], c["rack_of"], c["R"], 1)


def test_slot_0_is_never_exchanged_without_move_leaders():
    c = dx.leaders_only_case()
    moved = dx.run(c)
    assert moved["exchanges"] == 1 and moved["rows"][0, 0] == 1
    kept = dx.run(c, move_leaders=False)
    assert kept["kinds"] == "" and (kept["rows"] == c["rows"]).all() and kept["x_peak"] == 29
    exchanged = 0
    for seed in SEEDS:   # the family's kept-leader half: the restatement asserts the leaders every round; here that exchanges do happen there
        s = dr.small_case(seed)
        if not s["move_leaders"]:
            res = dx.run(s)
            assert (res["rows"][:, 0] == s["rows"][:, 0]).all()
            exchanged += res["exchanges"] > 0
    assert exchanged >= 10


def test_max_rounds_stops_before_between_and_at_the_end():
    c, full = _mid()
    kinds = full["kinds"]
    first_x = kinds.index("x")
    assert first_x >= 50 and "m" in kinds[first_x:] and kinds.endswith("xx") and not full["more"]
    early = dx.run(c, max_rounds=first_x - 3)                  # before the first exchange round: descend's bytes at that max_rounds
    plain = _plain(c, max_rounds=first_x - 3)
    assert early["rows"].tobytes() == plain["rows"].tobytes() and early["more"] and plain["more"] and early["x_peak"] == 0 and early["x_rounds"] == 0
    assert (early["rounds"], early["moves"], early["proposals"]) == (plain["rounds"], plain["moves"], plain["proposals"])
    edge = dx.run(c, max_rounds=first_x)                       # the moves are done: the probe is the first exchange round, and it has a proposal
    assert edge["rows"].tobytes() == _plain(c)["rows"].tobytes() and edge["more"] and edge["x_rounds"] == 0 and edge["x_peak"] == full["x_peak"] > 0
    at = len(kinds) - 20                                       # between two exchange rounds
    assert kinds[at - 1] == kinds[at] == "x"
    mid = dx.run(c, max_rounds=at)
    assert mid["more"] and mid["kinds"] == kinds[:at] and full["peak_after"] <= mid["peak_after"] <= full["x_peak"]
    assert mid["rows"].tobytes() != full["rows"].tobytes()
    last = dx.run(c, max_rounds=len(kinds))                    # exactly at the end: nothing is left, so nothing was stopped
    assert not last["more"] and last["rows"].tobytes() == full["rows"].tobytes() and last["kinds"] == kinds
    assert dx.run(c, max_rounds=len(kinds) - 1)["more"]


def test_mid_instance_reaches_the_bound_closely():
    """The table of section 4u: peak / bound 1.00208 -> 1.0000086 on (10, 2, 200, 3, 0.7, 7)."""
    c, full = _mid()
    lb, _ = dr.lower_bound(c["rows"], c["size"], c["B"])
    assert (full["rounds"], full["x_rounds"], full["exchanges"]) == (228, 142, 152)
    assert full["x_peak"] == _plain(c)["peak_after"] and round(full["x_peak"] / lb, 5) == 1.00208 and full["peak_after"] / lb < 1.00001
    assert full["x_lowered"] and full["shared"] >= 0
