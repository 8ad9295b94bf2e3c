"""The hole filling of an initialising k_search launch scores its candidates from band state: the partition's brokers are marked in W,
a rack table is built per hole, every index costs one W read, one RT read and a multiply-add, and the winner's counters and band rows
are brought up to date before the next hole is scanned (kao_search_dev.h: fill_hole).  It restates oracle/kao_port.c::ls_init -- same
holes in the same order, same winners -- so every launch must still replay the scalar restatement bit for bit.

Every case is replayed twice: one launch of ONE iteration, which shows the fill almost alone (the state, V and obj it leaves), and
three launches of 11 (the band state the fill leaves is what the iteration loop goes on from).  Compared: final state, best snapshot,
best_obj, V, obj, n_accept -- integers only, no tolerance.

The CPU half (no GPU needed) asserts that each case has the holes it claims -- holes, leader holes, partitions with two or more holes,
partitions with all slots empty, rounds per scan, and for the shrinking-RF case a winner that carries an objective weight -- so the GPU
half cannot pass vacuously."""
import dataclasses

import numpy as np
import pytest

from conftest import to_product_topic

RUNS = ((1, 1), (3, 11))      # (launches, iterations per launch)
NONE = 0xFFFF
_ENV_VARS = ("KAO_SEARCH_RFT", "KAO_SEARCH_SMALL", "KAO_CUR_GLOBAL", "KAO_INIT_WAVES")


def _tseed(seed, ti):
    return seed ^ (((ti + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def _oracle_topic(ko, pt):
    return ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                    n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights,
                    bounds_override=dict(pt.bounds_override))


def _old_rows(ko, B, R, P, RF):
    """The balanced assignment make_cluster starts from, in old broker ids (nothing removed: dense index = id)."""
    return np.asarray(ko.make_cluster("probe", B, R, 1, P, RF, [], []).topics[0].current).astype(int)


def _working(ot):
    """The words the fill starts from: current replicas in slots < RF, NONE elsewhere."""
    cur = np.asarray(ot.current).astype(int)
    a = np.full((ot.n_partitions, ot.rf), NONE, dtype=int)
    k = min(ot.rf, cur.shape[1])
    a[:, :k] = cur[:, :k]
    return a


def _shape(ot):
    hole = _working(ot) == NONE
    m = int(np.bincount(np.asarray(ot.rack_of).astype(int), minlength=ot.n_racks).max())
    sizes = np.bincount(np.asarray(ot.rack_of).astype(int), minlength=ot.n_racks)
    return dict(holes=int(hole.sum()), leader=int(hole[:, 0].sum()), multi=int((hole.sum(1) >= 2).sum()),
                all_empty=int(hole.all(1).sum()), lead_and_fol=int((hole[:, 0] & hole[:, 1:].any(1)).sum()),
                rounds=(ot.n_racks * m + 63) // 64, padding=int(ot.n_racks * m - sizes.sum()))


def _case(ko, name):
    """-> dict(ots, restarts, rhos, claims: lower bounds on _shape (rounds: exact), and optionally prices, team, env;
    rf3, small: the kernel and key form that must run)"""
    mk = ko.make_cluster
    if name == "rf3_two_rounds":      # 100 brokers / 10 racks / 20 partitions, 8 brokers removed: Bx = 100, the paired trip
        old = _old_rows(ko, 100, 10, 20, 3)
        rm = sorted({old[0, 0], old[1, 1], old[2, 2], old[3, 0], old[3, 1], old[5, 1], old[5, 2], old[7, 0]})
        assert len(rm) == 8
        ot = mk("t100", 100, 10, 1, 20, 3, rm, []).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 7), rf3=True, small=True, claims=dict(holes=8, leader=3, multi=2, lead_and_fol=1, rounds=2))
    if name == "rf3_three_rounds":    # 130 brokers on 4 racks of unequal size (33 / 33 / 28 / 31): Bx = 132, pair + remainder, padding inside
        old = _old_rows(ko, 130, 4, 20, 3)
        rm = sorted({2, 6, 10, 14, 3, int(old[0, 0]), int(old[4, 1]), int(old[4, 2])} - {0, 1})
        ot = mk("t130", 130, 4, 1, 20, 3, rm, []).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 7), rf3=True, small=True, claims=dict(holes=3, leader=1, multi=1, rounds=3, padding=5))
    if name == "all_slots_empty":     # 12 brokers / 3 racks / 4 partitions, partition 0's three replicas all removed: nothing to mark,
        old = _old_rows(ko, 12, 3, 4, 3)   # and slot 2's scan must see slot 1's winner
        ot = mk("p4e", 12, 3, 1, 4, 3, sorted(int(b) for b in old[0]), []).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 1, 4, 7), rf3=True, small=True, claims=dict(holes=3, leader=1, multi=1, all_empty=1, rounds=1))
    if name == "leader_and_follower":  # a partition with a leader hole and a follower hole: both passes write its row
        old = _old_rows(ko, 40, 4, 30, 3)
        ot = mk("b40", 40, 4, 1, 30, 3, sorted({int(old[2, 0]), int(old[2, 1]), int(old[9, 2])}), [(40, 2), (41, 3)]).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 1, 4, 7), rf3=True, small=True, claims=dict(holes=3, leader=1, multi=1, lead_and_fol=1, rounds=1))
    if name == "general_keys":        # the clamp
        return dict(_case(ko, "rf3_two_rounds"), small=False, env={"KAO_SEARCH_SMALL": "0"})
    if name == "wide_replica_band":   # replica band 4 wide (six table entries): the form with arithmetic rows
        ot = mk("o3", 30, 3, 1, 20, 3, [4, 17], [(30, 1)], bounds_override={"rep_lo": 1, "rep_hi": 4, "prack_lo": 1, "prack_hi": 2}).topics[0]
        bd = ot.bounds()
        assert (bd["rep_lo"], bd["rep_hi"], bd["prack_lo"], bd["prack_hi"]) == (1, 4, 1, 2)
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 7), rf3=True, small=False, claims=dict(holes=2, leader=1, rounds=1))
    if name in ("rf2", "rf5"):        # the generic kernel, four and eight words per partition, RF read per topic
        rf = int(name[2])
        old = _old_rows(ko, 90, 6, 40, rf)
        ot = mk(name, 90, 6, 1, 40, rf, sorted({int(old[0, 1]), int(old[0, rf - 1]), int(old[5, 0]), int(old[11, 0]), 31, 77}), [(90, 1), (91, 5)]).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 2, 5), rf3=False, small=False, claims=dict(holes=3, leader=1, rounds=2, **({"multi": 1} if rf == 5 else {})))   # (RF 2: partition 0 has one hole)
    if name == "shrinking_rf":        # current RF 4, RF 3: the dropped fourth replica is a candidate with an objective weight
        old = _old_rows(ko, 40, 4, 24, 4)
        ot = mk("shr", 40, 4, 1, 24, 4, sorted({int(old[0, 0]), int(old[3, 1]), int(old[3, 2]), int(old[8, 0]), int(old[13, 1])}), [(40, 1)], new_rf=3).topics[0]
        assert ot.rf == 3 and ot.current.shape[1] == 4
        return dict(ots=[ot], restarts=8, rhos=(1, 2, 4), rf3=False, small=False, claims=dict(holes=4, leader=1, multi=1, rounds=1))
    if name == "priced_broker_weights":   # priced launch with BW: the priced terms and hbw
        ot = mk("b100", 100, 5, 1, 60, 3, [3, 50, 97], [(100, 0), (101, 4)]).topics[0]
        rng = np.random.default_rng(31)
        ot = dataclasses.replace(ot, broker_w=rng.integers(0, 4, ot.n_brokers).astype(np.int32), broker_wl=rng.integers(0, 3, ot.n_brokers).astype(np.int32))
        prices = [(rng.integers(-8, 9, ot.n_brokers).astype(np.int32) * 16384, rng.integers(-4, 5, ot.n_brokers).astype(np.int32) * 16384,
                   rng.integers(-2, 3, ot.n_racks).astype(np.int32) * 16384)]
        return dict(ots=[ot], restarts=4, rhos=(0, 3), prices=prices, rf3=False, small=False, claims=dict(holes=4, leader=1, rounds=2))
    if name == "global_memory":       # the in-kernel fill on a topic in global memory (KAO_INIT_WAVES=0: no K-init launch in front)
        from kafka_assignment_optimizer_amd import synthetic as sy
        pts = sy.drift(sy.make_cluster(1000, 20, 1, 6000, 3, [7, 77, 777], [(1000, 7), (1001, 17), (1002, 17)]), 0.2, 3)
        return dict(ots=[_oracle_topic(ko, pts[0])], restarts=3, rhos=(0, 2), team=1, env={"KAO_CUR_GLOBAL": "0", "KAO_INIT_WAVES": "0"},
                    rf3=False, small=False, claims=dict(holes=20, leader=5, rounds=16))
    if name == "team_of_four":        # the same with a team: its first wavefront fills, the marks go into the team's shared W
        return dict(_case(ko, "global_memory"), team=4, env={"KAO_INIT_WAVES": "0"})
    raise KeyError(name)


CASES = ["rf3_two_rounds", "rf3_three_rounds", "all_slots_empty", "leader_and_follower", "general_keys", "wide_replica_band", "rf2", "rf5",
         "shrinking_rf", "priced_broker_weights", "global_memory", "team_of_four"]
_REFS = {}


def _seed(name):
    return 0x1A17 + 811 * CASES.index(name)


def _refs(ko, kp, name):
    """The scalar restatement of every (run, topic, restart) of the case, computed once and shared by both halves."""
    if name not in _REFS:
        case = _case(ko, name)
        out = {}
        for launches, iters in RUNS:
            for ti, ot in enumerate(case["ots"]):
                for rho in case["rhos"]:
                    if case.get("prices") is None:
                        out[(launches, ti, rho)] = kp.port_search(ot, _tseed(_seed(name), ti), rho, launches, iters, team=max(1, case.get("team", 0)))
                    else:   # (priced launches: the same restatement, launch by launch)
                        run = kp.PortRun(ot, _tseed(_seed(name), ti), rho)
                        for ln in range(launches):
                            run.launch(ln, iters, prices=case["prices"][ti])
                        out[(launches, ti, rho)] = run.read()
                        run.close()
        _REFS[name] = (case, out)
    return _REFS[name]


@pytest.mark.parametrize("name", CASES)
def test_case_has_the_holes_it_claims(ko, kp, name):
    """CPU half: holes, leader holes, partitions with several holes / with every slot empty, rounds per scan; the restatement fills them."""
    case, refs = _refs(ko, kp, name)
    for ot in case["ots"]:
        sh = _shape(ot)
        print(name, sh)
        for key, want in case["claims"].items():
            if key == "rounds" and name not in ("global_memory", "team_of_four"):
                assert sh[key] == want, (name, key, sh)
            else:
                assert sh[key] >= want, (name, key, sh)
        if case["rf3"]:
            assert ot.rf == 3 and ot.current.shape[1] <= 3
    # the fill leaves no hole, and keeps every surviving replica of a slot < RF where it was
    for (launches, ti, rho), ref in refs.items():
        assert (ref["final"] != NONE).all(), (name, launches, rho)
    if name == "shrinking_rf":
        # a winner that carries a weight: a hole filled with the partition's dropped fourth replica.  (The fill alone: no iteration.)
        ot = case["ots"][0]
        cur, work = np.asarray(ot.current).astype(int), _working(ot)
        for rho in case["rhos"]:
            fin = kp.port_search(ot, _tseed(_seed(name), 0), rho, 1, 0)["final"].astype(int)
            carried = sum(int(work[p, k] == NONE and cur[p, 3] != NONE and fin[p, k] == cur[p, 3]) for p in range(ot.n_partitions) for k in range(3))
            print("restart", rho, "holes filled with the dropped current replica:", carried)
            assert carried >= 1, rho


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_init_replay_bit_exact(kao, ko, kp, monkeypatch, name):
    """GPU half: one launch of one iteration and three launches of 11 against the restatement, through the kernel and key form the case names."""
    case, refs = _refs(ko, kp, name)
    for var in _ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in case.get("env", {}).items():
        monkeypatch.setenv(var, val)
    for launches, iters in RUNS:
        opts = dict(seed=_seed(name), restarts=case["restarts"], iters_per_launch=iters)
        if "team" in case:
            opts["team"] = case["team"]
        with kao.Session([to_product_topic(t) for t in case["ots"]], **opts) as s:
            if case.get("prices") is not None:
                for ti, pr in enumerate(case["prices"]):
                    s.set_prices(ti, *pr)
            s.step(launches)
            st = s.stats()
            assert st["drift"] == 0
            assert st["search_rf3_launches"] == (launches * st["launch_groups"] if case["rf3"] else 0)
            assert s.small_launches() == (launches * st["launch_groups"] if case["small"] else 0)
            devs = {key: s.restart_state(*key[1:]) for key in refs if key[0] == launches}
        for key, dev in devs.items():
            ref = refs[key]
            assert dev["final"].tolist() == ref["final"].tolist(), (name, key)
            assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (name, key)
            if ref["best_obj"] >= 0:
                assert dev["best"].tolist() == ref["best"].tolist(), (name, key)
