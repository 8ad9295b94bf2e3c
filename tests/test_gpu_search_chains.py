"""k_search issues the LDS reads of independent work together (kao_search.hip, kao_search_dev.h): a trip of two scan rounds reads both
rounds' W / XR words and then both RT words -- in the fused two-slot scan, in the one-slot scan and in the hole filling -- and an
accepted move updates its counters one lane each in one round trip (the small-cost instantiations; the others keep one
read-modify-write after the other).  Draws, keys, winners, stores and counters are those of oracle/kao_port.c: every case is replayed
bit for bit -- final state, best snapshot, best_obj, V, obj, n_accept -- at three launches of 5, of 11 and of 19 iterations.

The cases are the smallest shapes at which that code can go wrong: one round (no pair), exactly two, pair + remainder, four pairs + one
round, the clamped keys, the one-slot scan (a priced launch keeps it), weighted rounds in front of, behind and between pairs, every
kind of accepted move, one rack, one partition, and one case for each generic instantiation that shares the edited code.

The CPU half (no GPU needed) asserts from the scalar restatement that each case contains what it claims: the rounds per scan, and --
from the accepted moves of the first launch of 19 iterations, found by replaying it iteration by iteration -- the kinds of move and
where the displaced current replicas of a scanned partition fall, so the GPU half cannot pass vacuously."""
import dataclasses

import numpy as np
import pytest

from conftest import to_product_topic

ITERS = (5, 11, 19)           # iterations per launch; every run is three launches
LAUNCHES = 3
TRACE = 19                    # the first launch of the 19-iteration run is taken apart move by move
NONE = 0xFFFF
_ENV_VARS = ("KAO_SEARCH_RFT", "KAO_SEARCH_SMALL", "KAO_CUR_GLOBAL", "KAO_INIT_WAVES")
MOVE_KINDS = ("replace_in_rack", "replace_follower_across", "replace_leader_across", "exchange_leader_follower", "exchange_same_kind", "leader_swap")


def _tseed(seed, ti):
    return seed ^ (((ti + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def _oracle_topic(ko, pt):
    return ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                    n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights,
                    bounds_override=dict(pt.bounds_override))


def _old_rows(ko, B, R, P, RF):
    """The balanced assignment make_cluster starts from, in old broker ids (nothing removed: dense index = id)."""
    return np.asarray(ko.make_cluster("probe", B, R, 1, P, RF, [], []).topics[0].current).astype(int)


def _drifted(ko, B, R, P, RF, removed, added, frac, seed):
    """make_cluster, then `frac` of the replica slots moved to random brokers (synthetic.drift): the search moves them back and on, so
    partitions soon hold fewer of their current replicas than they have -- the displaced ones are what a scan scores with weights."""
    from kafka_assignment_optimizer_amd import synthetic as sy
    return _oracle_topic(ko, sy.drift(sy.make_cluster(B, R, 1, P, RF, removed, added), frac, seed)[0])


def _index_space(ot):
    """-> (internal index of every broker, rounds per scan): rack-major, stride m = the largest rack (at least 2), brokers of a rack in
    ascending order (oracle/kao_port.c, kao_model.cpp)."""
    racks = np.asarray(ot.rack_of).astype(int)
    m = max(2, int(np.bincount(racks, minlength=ot.n_racks).max()))
    fill = [0] * ot.n_racks
    x = np.zeros(len(racks), dtype=int)
    for b, r in enumerate(racks):
        x[b] = r * m + fill[r]
        fill[r] += 1
    return x, (ot.n_racks * m + 63) // 64


def _case(ko, name):
    """-> dict(ots, restarts, rhos, rounds (exact; None: not asserted), claims: what the first launch of TRACE iterations must contain,
    and optionally prices, team, env; rf3, small: the kernel and key form that must run)"""
    mk = ko.make_cluster
    if name == "one_round":           # 12 brokers / 3 racks: Bx = 12, a remainder round and no pair
        ot = _drifted(ko, 12, 3, 8, 3, [2], [(12, 2)], 0.3, 1)
        return dict(ots=[ot], restarts=8, rhos=(0, 1, 4, 7), rf3=True, small=True, rounds=1, claims=("replace_in_rack", "replace_follower_across", "replace_leader_across", "leader_swap"))
    if name == "two_rounds":          # 100 brokers / 10 racks / 20 partitions, 8 removed: Bx = 100, exactly one pair, padding inside
        old = _old_rows(ko, 100, 10, 20, 3)
        rm = sorted({old[0, 0], old[1, 1], old[2, 2], old[3, 0], old[3, 1], old[5, 1], old[5, 2], old[7, 0]})
        ot = _drifted(ko, 100, 10, 20, 3, [int(b) for b in rm], [], 0.3, 2)
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 5, 7), rf3=True, small=True, rounds=2, claims=("w_round0", "w_last"))
    if name == "three_rounds":        # 130 brokers on 4 racks of unequal size: Bx = 132, pair + remainder (a read ahead would pass the end)
        old = _old_rows(ko, 130, 4, 20, 3)
        rm = sorted({2, 6, 10, 14, 3, int(old[0, 0]), int(old[4, 1]), int(old[4, 2])} - {0, 1})
        ot = _drifted(ko, 130, 4, 20, 3, rm, [], 0.3, 3)
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 5, 7), rf3=True, small=True, rounds=3, claims=("w_round0", "w_adjacent"))
    if name == "nine_rounds":         # 9 racks x 64: four pairs, then a single round
        old = _old_rows(ko, 576, 9, 30, 3)
        rm = sorted({int(old[0, 0]), int(old[1, 1]), int(old[2, 2]), int(old[3, 0]), int(old[3, 1]), int(old[6, 2])})
        ot = _drifted(ko, 576, 9, 30, 3, rm, [], 0.3, 4)
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 5, 7), rf3=True, small=True, rounds=9, claims=("w_inner",))
    if name == "two_rounds_general":  # the same pair with clamped keys
        return dict(_case(ko, "two_rounds"), small=False, env={"KAO_SEARCH_SMALL": "0"})
    if name == "one_slot_scan":       # a priced launch keeps the slot-by-slot scan (as tests/test_gpu_scan_two.py forces it): pair + remainder
        base = _case(ko, "three_rounds")
        rng = np.random.default_rng(17)
        ot = base["ots"][0]
        prices = [(rng.integers(-8, 9, ot.n_brokers).astype(np.int32) * 16384, rng.integers(-4, 5, ot.n_brokers).astype(np.int32) * 16384,
                   rng.integers(-2, 3, ot.n_racks).astype(np.int32) * 16384)]
        return dict(base, prices=prices, rf3=False, small=False, restarts=4, rhos=(0, 3), claims=())
    if name == "moves_of_every_kind":  # 40 brokers / 4 racks / 30 partitions: one round, many accepted moves of every kind
        old = _old_rows(ko, 40, 4, 30, 3)
        ot = mk("b40", 40, 4, 1, 30, 3, sorted({int(old[2, 0]), int(old[2, 1]), int(old[9, 2]), 1, 7, 13}), [(40, 2), (41, 3)]).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 1, 2, 3, 4, 5, 6, 7), rf3=True, small=True, rounds=1, claims=MOVE_KINDS)
    if name == "one_rack":            # every REPLACE stays inside the rack: the rack totals are never touched
        ot = mk("r1", 20, 1, 1, 12, 3, [3, 11], [(20, 0)]).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 2, 5), rf3=True, small=True, rounds=1, claims=("replace_in_rack",), never=("replace_follower_across", "replace_leader_across"))
    if name == "one_partition":       # no EXCHANGE partner; both scan slots lie in the one partition: their displaced replicas share a round
        ot = _drifted(ko, 12, 3, 1, 3, [0], [(12, 0)], 0.7, 14)   # (two replicas in one rack: one has to leave, and stays displaced)
        return dict(ots=[ot], restarts=8, rhos=(0, 1, 2, 3, 4, 5, 6, 7), rf3=True, small=True, rounds=1, claims=("w_both_slots", "replace_leader_across", "leader_swap"), never=("exchange_leader_follower", "exchange_same_kind"))
    if name in ("rf2", "rf5"):        # the generic kernel, four and eight words per partition, RF read per topic
        rf = int(name[2])
        old = _old_rows(ko, 90, 6, 40, rf)
        ot = mk(name, 90, 6, 1, 40, rf, sorted({int(old[0, 1]), int(old[0, rf - 1]), int(old[5, 0]), int(old[11, 0]), 31, 77}), [(90, 1), (91, 5)]).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 2, 5), rf3=False, small=False, rounds=2, claims=())
    if name == "priced_broker_weights":   # priced with broker weights: the one-slot scan with BW, finish in the generic form
        ot = mk("b100", 100, 5, 1, 60, 3, [3, 50, 97], [(100, 0), (101, 4)]).topics[0]
        rng = np.random.default_rng(31)
        ot = dataclasses.replace(ot, broker_w=rng.integers(0, 4, ot.n_brokers).astype(np.int32), broker_wl=rng.integers(0, 3, ot.n_brokers).astype(np.int32))
        prices = [(rng.integers(-8, 9, ot.n_brokers).astype(np.int32) * 16384, rng.integers(-4, 5, ot.n_brokers).astype(np.int32) * 16384,
                   rng.integers(-2, 3, ot.n_racks).astype(np.int32) * 16384)]
        return dict(ots=[ot], restarts=4, rhos=(0, 3), prices=prices, rf3=False, small=False, rounds=2, claims=())
    if name == "global_memory":       # a topic in global memory (KAO_INIT_WAVES=0: the in-kernel fill, whose pairs are edited too)
        from kafka_assignment_optimizer_amd import synthetic as sy
        pts = sy.drift(sy.make_cluster(1000, 20, 1, 6000, 3, [7, 77, 777], [(1000, 7), (1001, 17), (1002, 17)]), 0.2, 3)
        return dict(ots=[_oracle_topic(ko, pts[0])], restarts=3, rhos=(0, 2), team=1, env={"KAO_CUR_GLOBAL": "0", "KAO_INIT_WAVES": "0"},
                    rf3=False, small=False, rounds=None, claims=())
    if name == "team_of_four":        # the same with a team: finish keeps the form its record exchange orders
        return dict(_case(ko, "global_memory"), team=4, env={"KAO_INIT_WAVES": "0"})
    raise KeyError(name)


CASES = ["one_round", "two_rounds", "three_rounds", "nine_rounds", "two_rounds_general", "one_slot_scan", "moves_of_every_kind", "one_rack",
         "one_partition", "rf2", "rf5", "priced_broker_weights", "global_memory", "team_of_four"]
_REFS, _TRACES = {}, {}


def _seed(name):
    return 0xC4A17 + 811 * CASES.index(name)


def _replay(kp, case, name, ti, ot, rho, launches, iters):
    team = max(1, case.get("team", 0))
    if case.get("prices") is None:
        return kp.port_search(ot, _tseed(_seed(name), ti), rho, launches, iters, team=team)
    run = kp.PortRun(ot, _tseed(_seed(name), ti), rho)   # (priced launches: the same restatement, launch by launch)
    for ln in range(launches):
        run.launch(ln, iters, prices=case["prices"][ti])
    out = run.read()
    run.close()
    return out


def _refs(ko, kp, name):
    """The scalar restatement of every (iterations, topic, restart) of the case, computed once and shared by both halves."""
    if name not in _REFS:
        case = _case(ko, name)
        _REFS[name] = (case, {(iters, ti, rho): _replay(kp, case, name, ti, ot, rho, LAUNCHES, iters)
                              for iters in ITERS for ti, ot in enumerate(case["ots"]) for rho in case["rhos"]})
    return _REFS[name]


def _trace(ko, kp, name):
    """What the first launch of TRACE iterations does, move by move: a launch of i iterations is the first i iterations of a longer
    first launch (same generator key, same penalty schedule), so the move of iteration i is the difference between the states after i
    and after i + 1.  -> Counter of MOVE_KINDS and of where the displaced current replicas of a scanned partition fall."""
    if name in _TRACES:
        return _TRACES[name]
    import collections
    case, _ = _refs(ko, kp, name)
    found = collections.Counter()
    for ti, ot in enumerate(case["ots"]):
        racks, cur = np.asarray(ot.rack_of).astype(int), np.asarray(ot.current).astype(int)
        xs, n_rd = _index_space(ot)
        for rho in case["rhos"]:
            prev = _replay(kp, case, name, ti, ot, rho, 1, 0)
            for it in range(TRACE):
                nxt = _replay(kp, case, name, ti, ot, rho, 1, it + 1)
                a, b = prev["final"].astype(int), nxt["final"].astype(int)
                cells = np.argwhere(a != b)
                assert nxt["n_accept"] - prev["n_accept"] == (1 if len(cells) else 0), (name, rho, it)
                kind = (0x1210 >> ((it & 7) * 2)) & 3   # R R X R L R X R
                sampled = kind == 2 or (kind == 0 and (it >> 3) & 1)
                if len(cells) == 1:
                    assert kind == 0
                    p, k = (int(v) for v in cells[0])
                    same = racks[a[p, k]] == racks[b[p, k]]
                    found["replace_in_rack" if same else ("replace_leader_across" if k == 0 else "replace_follower_across")] += 1
                    if not sampled:   # a scan of slot (p, k): the current replicas of p that its words do not hold are scored with weights
                        rds = sorted(int(xs[c]) >> 6 for c in cur[p] if c != NONE and c not in a[p])
                        found["w_round0"] += int(n_rd > 1 and 0 in rds)
                        found["w_last"] += int(n_rd > 1 and n_rd - 1 in rds)
                        found["w_adjacent"] += int(any(r + 1 in rds for r in rds))
                        found["w_inner"] += int(any(0 < r < n_rd - 1 for r in rds))
                        found["w_both_slots"] += int(ot.n_partitions == 1 and len(rds) > 0 and case.get("prices") is None)
                elif len(cells) == 2:
                    (p, k), (q, j) = ((int(v) for v in c) for c in cells)
                    assert a[p, k] == b[q, j] and a[q, j] == b[p, k], (name, rho, it)
                    if p == q:
                        assert kind == 2 and k == 0
                        found["leader_swap"] += 1
                    else:
                        assert kind == 1
                        found["exchange_leader_follower" if (k == 0) != (j == 0) else "exchange_same_kind"] += 1
                else:
                    assert len(cells) == 0, (name, rho, it, cells)
                prev = nxt
    _TRACES[name] = found
    return found


@pytest.mark.parametrize("name", CASES)
def test_case_contains_what_it_claims(ko, kp, name):
    """CPU half: rounds per scan, the kinds of accepted move and the positions of the weighted rounds, from the restatement."""
    case, refs = _refs(ko, kp, name)
    for ot in case["ots"]:
        if case["rounds"] is not None:
            assert _index_space(ot)[1] == case["rounds"], (name, _index_space(ot)[1])
        if case["rf3"]:
            assert ot.rf == 3 and ot.current.shape[1] <= 3
    assert sum(ref["n_accept"] for ref in refs.values()) > 0, name
    if case.get("team", 0) > 1:   # (a team applies several moves per iteration: not taken apart)
        return
    if not case["claims"] and not case.get("never"):
        return
    found = _trace(ko, kp, name)
    print(name, dict(found))
    for key in case["claims"]:
        assert found[key] >= 1, (name, key, dict(found))
    for key in case.get("never", ()):
        assert found[key] == 0, (name, key, dict(found))


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_chains_replay_bit_exact(kao, ko, kp, monkeypatch, name):
    """GPU half: three launches of 5, of 11 and of 19 iterations against the restatement, through the kernel and key form the case names."""
    case, refs = _refs(ko, kp, name)
    for var in _ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in case.get("env", {}).items():
        monkeypatch.setenv(var, val)
    for iters in ITERS:
        opts = dict(seed=_seed(name), restarts=case["restarts"], iters_per_launch=iters)
        if "team" in case:
            opts["team"] = case["team"]
        with kao.Session([to_product_topic(t) for t in case["ots"]], **opts) as s:
            if case.get("prices") is not None:
                for ti, pr in enumerate(case["prices"]):
                    s.set_prices(ti, *pr)
            s.step(LAUNCHES)
            st = s.stats()
            assert st["drift"] == 0
            assert st["search_rf3_launches"] == (LAUNCHES * st["launch_groups"] if case["rf3"] else 0)
            assert s.small_launches() == (LAUNCHES * st["launch_groups"] if case["small"] else 0)
            devs = {key: s.restart_state(*key[1:]) for key in refs if key[0] == iters}
        for key, dev in devs.items():
            ref = refs[key]
            assert dev["final"].tolist() == ref["final"].tolist(), (name, key)
            assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (name, key)
            if ref["best_obj"] >= 0:
                assert dev["best"].tolist() == ref["best"].tolist(), (name, key)
