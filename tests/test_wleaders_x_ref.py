"""CPU tests of the weighted leader balance with exchange moves (kao_balance_leaders_weighted_exchange): the
restatement in tests/wleaders_x_ref.py (which asserts, every round, that winners share no broker, that no partition is touched twice,
that the lowest key wins, that the peak never rises and the sum of squares falls by 2 delta (D - delta), and on these sizes that its
partner search is complete against all pairs) on the small family, on equal weights, on the hand-built completeness case and at the
three max_rounds edges."""
import numpy as np
import pytest

import wleaders_ref as wr
import wleaders_x_ref as xr

NONE = 0xFFFF
SEEDS = range(120)


@pytest.fixture(scope="module")
def family():
    """Per seed: the instance, the plain restatement, the exchange restatement, the optimum."""
    out = []
    for seed in SEEDS:
        rows, weight, B = wr.small_case(seed)
        out.append((rows, weight, B, wr.descend(rows, weight, B), xr.descend(rows, weight, B), wr.optimum(rows, weight, B)))
    return out


def test_small_family_is_bracketed_stable_and_starts_from_the_plain_end_state(family):
    """lower_bound <= optimum <= peak_exchange <= peak_plain <= peak_before; the state at the first exchange round is the plain
    call's end state; the end state is move-stable and, against all pairs, exchange-stable.  The counts are what the restatement
    gives: pinned, so that an exchange round that does nothing cannot pass."""
    at_opt_x = at_opt_plain = lower = higher = x_rounds = exchanges = proven_x = proven_plain = 0
    for seed, (rows, weight, B, plain, res, opt) in enumerate(family):
        lb, _ = wr.lower_bound(res["rows"], weight, B)
        assert lb <= opt <= res["peak_after"] <= plain["peak_after"] <= res["peak_before"] == plain["peak_before"], seed
        assert (res["first_x"] == plain["lead"]).all(), seed
        assert wr.stable(rows, res["rows"], weight, B) and xr.exchange_stable(res["rows"], weight, B), seed
        assert not res["more"] and res["peak_after"] == int(wr.loads(res["rows"], weight, B).max()), seed
        assert res["n_changed"] == int((res["rows"] != rows).any(axis=1).sum()), seed
        assert res["rounds"] >= plain["rounds"] + res["x_rounds"], seed   # move rounds can follow an exchange round
        assert res["moves"] >= res["rounds"] and res["exchanges"] >= res["x_rounds"] and res["x_proposals"] >= res["exchanges"], seed
        if res["x_rounds"] == 0:
            assert res["rows"].tobytes() == plain["rows"].tobytes(), seed
        at_opt_x += res["peak_after"] == opt
        at_opt_plain += plain["peak_after"] == opt
        lower += res["peak_after"] < plain["peak_after"]
        higher += res["peak_after"] > plain["peak_after"]
        x_rounds += res["x_rounds"]
        exchanges += res["exchanges"]
        proven_x += res["peak_after"] == lb
        proven_plain += plain["peak_after"] == wr.lower_bound(plain["rows"], weight, B)[0]
    print(f"peak==optimum: {at_opt_x} with exchanges, {at_opt_plain} plain; strictly lower: {lower}; exchange rounds: {x_rounds}; exchanges: "
          f"{exchanges}; proven: {proven_x} against {proven_plain}")
    assert lower >= 1 and higher == 0   # the conditions
    assert (at_opt_x, at_opt_plain, lower, x_rounds) == (65, 52, 40, 111)   # the pins
    assert (exchanges, proven_x, proven_plain) == (122, 37, 32)


def test_exchange_stability_check_sees_an_open_pair(family):
    """The brute-force check is not vacuous: the plain call's end state fails it on the seeds where an exchange round ran."""
    open_pairs = 0
    for rows, weight, B, plain, res, _ in family:
        if res["x_rounds"]:
            assert not xr.exchange_stable(plain["rows"], weight, B)
            open_pairs += 1
        else:
            assert xr.exchange_stable(plain["rows"], weight, B)
    assert open_pairs >= 1


def test_equal_positive_weights_give_the_plain_restatement_s_bytes():
    for seed in list(range(0, 120, 10)) + [3, 7]:
        rows, weight, B = wr.small_case(seed)
        w = weight if seed % 10 == 0 else np.where(weight > 0, 9, 0).astype(np.int64)   # zeros stay zeros: the positive ones are equal
        plain, res = wr.descend(rows, w, B), xr.descend(rows, w, B)
        assert res["x_rounds"] == 0 and res["exchanges"] == 0
        assert res["rows"].tobytes() == plain["rows"].tobytes()
        assert [res[k] for k in ("rounds", "moves", "proposals", "n_changed", "peak_after")] == [plain[k] for k in ("rounds", "moves", "proposals", "n_changed", "peak_after")]


def forced_case():
    """The only passing partner lies on the heavy side of the split, and 2 min_gain >= D: W(0) = 573, W(1) = 523, D = 50, min_gain = 30.
    x = partition 0 (100, led by 0).  Led by 1 on the same pair: 120 and 100 (delta <= 0), 95 (delta 5: passes, 5 + 30 < 50), 78 (delta
    22: before the split at delta 25, fails 22 + 30 < 50, and sits between the split and the partner), 70 and 60 (after the split:
    fail).  No move is left: 523 + 100 + 30 >= 573.  The unclamped midpoint 100 - 25 = 75 has 78 and 70 as its neighbours: neither
    passes."""
    rows = np.array([[0, 1], [1, 0], [1, 0], [1, 0], [1, 0], [1, 0], [1, 0], [0, NONE]], dtype=np.int64)
    weight = np.array([100, 120, 100, 95, 78, 70, 60, 473], dtype=np.int64)
    return rows, weight, 2, 30


def test_forced_completeness_case_finds_the_exchange():
    rows, weight, B, mg = forced_case()
    D = 573 - 523
    assert 2 * mg >= D and [w for w in weight[1:7] if 0 < 100 - w and 100 - w + mg < D] == [95]
    plain, res = wr.descend(rows, weight, B, mg), xr.descend(rows, weight, B, mg)
    assert plain["rounds"] == 0 and plain["n_changed"] == 0
    assert (res["x_rounds"], res["exchanges"], res["x_proposals"], res["n_changed"]) == (1, 1, 1, 2)
    assert res["lead"].tolist() == [1, 0, 0, 1, 0, 0, 0, 0] and (res["peak_before"], res["peak_after"]) == (573, 568)
    assert xr.exchange_stable(res["rows"], weight, B, mg) and not xr.exchange_stable(rows, weight, B, mg)


def test_max_rounds_edges_set_the_more_flag():
    """The stop in the move phase, exactly before the first exchange round, inside the exchange phase, and at the very end."""
    rows, weight = wr.lognormal_case(6, 300, 3, 0.7, 7)
    full, plain = xr.descend(rows, weight, 6), wr.descend(rows, weight, 6)
    moves = plain["rounds"]
    assert full["x_rounds"] >= 3 and full["rounds"] > moves + 2 and (full["first_x"] == plain["lead"]).all()
    for limit, x_rounds, more in ((moves - 1, 0, True), (moves, 0, True), (moves + 1, 1, True), (full["rounds"] - 1, None, True),
                                  (full["rounds"], full["x_rounds"], False), (full["rounds"] + 5, full["x_rounds"], False)):
        res = xr.descend(rows, weight, 6, max_rounds=limit)
        assert res["rounds"] == min(limit, full["rounds"]) and res["more"] is more, limit
        if x_rounds is not None:
            assert res["x_rounds"] == x_rounds, limit
        assert plain["peak_before"] >= res["peak_after"] >= full["peak_after"]
        if limit == moves:   # the plain call's end state, with an exchange proposal left
            assert res["rows"].tobytes() == plain["rows"].tobytes() and wr.descend(rows, weight, 6, max_rounds=limit)["more"] is False
    no_x = xr.descend(rows, weight, 6, exchange=False)
    assert no_x["rows"].tobytes() == plain["rows"].tobytes() and no_x["x_rounds"] == 0


def test_batch_boundary_case_takes_exactly_one_batch_of_rounds():
    """tests/test_gpu_wleaders_x.py relies on it: 32 rounds of both kinds, the batch of the multi-launch path, so its last round with
    a proposal is the last of a batch."""
    res = xr.descend(*wr.lognormal_case(5, 120, 3, 0.7, 28), 5)
    assert (res["rounds"], res["x_rounds"]) == (32, 13) and not res["more"]


def test_pair_index_holds_every_pair_once_in_weight_order():
    rows, weight, B = wr.small_case(5)
    pi, segs = xr.pair_index(rows, weight)
    assert sorted(pi.tolist()) == list(range(len(rows))) and all(weight[a] > weight[b] or (weight[a] == weight[b] and a < b) for a, b in zip(pi[:-1], pi[1:]))
    want = {}
    for p, r in enumerate(rows.tolist()):
        held = [b for b in r if b != NONE]
        for i in held:
            for j in held:
                if i < j and weight[p] > 0:
                    want.setdefault((i, j), set()).add(p)
    assert {k: set(v.tolist()) for k, v in segs.items()} == want
    place = {p: i for i, p in enumerate(pi.tolist())}
    assert all([place[p] for p in v.tolist()] == sorted(place[p] for p in v.tolist()) for v in segs.values())
