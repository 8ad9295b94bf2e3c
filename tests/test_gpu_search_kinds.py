"""Every move kind of k_search's iteration ends in its own apply code (fused two-slot REPLACE scan, one-slot REPLACE scan, sampled
REPLACE, EXCHANGE, LEADER-SWAP).  Replayed bit for bit against the scalar restatement (oracle/kao_port.c): restart states, best
snapshots, V, objective and accepted-move counts.

The move kind follows a cycle of 16 iterations (R R X R L R X R, the REPLACEs scanned in the first half and sampled in the second).
Sessions of 5, 11 and 19 iterations per launch, three launches each, start and end their launches in every phase of that cycle, so
each kind's apply code is the last thing before an end-of-launch recount (the kernel's drift counter) and the first after a reload.

Cases: one per instantiation launch_search dispatches -- the RF-3 kernel, the generic one with four words per partition (RF 2 and
RF 4) and with eight (RF 5), priced, wide (512 replica slots or more), working words in LDS with the current assignment in global
memory (k_search_curg), topics in global memory, a team -- and two edge inputs where a kind has no candidate and its iterations are
skipped: a one-partition topic (no EXCHANGE partner) and RF 1 (no LEADER-SWAP).

The CPU half (no GPU needed) checks that the restatement accepts moves on every topic of every case and that its incremental V and
objective equal a from-scratch evaluation of the final state (the restatement's own drift check), so the GPU half cannot pass
vacuously.  Integer replays: nothing is compared with a tolerance."""
import numpy as np
import pytest

from conftest import to_product_topic

ITERS = (5, 11, 19)
LAUNCHES = 3


def _tseed(seed, ti):
    return seed ^ (((ti + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def _oracle_topic(ko, pt):
    return ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                    n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights,
                    bounds_override=dict(pt.bounds_override))


def _synthetic(ko, B, R, P, rf, removed, added, drift_seed):
    from kafka_assignment_optimizer_amd import synthetic as sy
    pts = sy.make_cluster(B, R, 1, P, rf, removed, added)
    if drift_seed:
        pts = sy.drift(pts, 0.2, drift_seed)
    return [_oracle_topic(ko, pts[0])]


def _prices(ots, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(-8, 9, t.n_brokers).astype(np.int32) * 16384, rng.integers(-4, 5, t.n_brokers).astype(np.int32) * 16384,
             rng.integers(-2, 3, t.n_racks).astype(np.int32) * 16384) for t in ots]


def _case(ko, name):
    """-> dict(ots, restarts, rhos, and optionally prices, team, env, rf3 (every launch through the RF-3 kernel, or none), check(stats))"""
    mk = ko.make_cluster
    if name == "rf3":          # the benchmark's shape: 50 partitions, RF 3, 500 brokers on 10 racks, drifted -- the fused two-slot scan
        from kafka_assignment_optimizer_amd import synthetic as sy
        ots = [_oracle_topic(ko, pt) for pt in sy.drift(sy.make_config(4, n_topics=2), 0.2, 1)]
        assert all(t.rf == 3 and t.n_partitions == 50 and t.n_brokers == 500 for t in ots)
        return dict(ots=ots, restarts=8, rhos=(0, 3, 7), rf3=True)
    if name == "rf3_generic":  # the same topics through the generic four-word kernel
        return dict(_case(ko, "rf3"), rf3=False, env={"KAO_SEARCH_RFT": "0"})
    if name in ("rf2", "rf4", "rf5"):   # four words per partition at RF 2 and RF 4, eight at RF 5
        rf = int(name[2])
        return dict(ots=[mk(name, 90, 6, 1, 40, rf, [4, 31, 77], [(90, 1), (91, 5)]).topics[0]], restarts=8, rhos=(0, 2, 5), rf3=False)
    if name == "priced":
        ots = [mk("b100", 100, 5, 1, 60, 3, [3, 50, 97], [(100, 0), (101, 4)]).topics[0],
               mk("b170", 170, 7, 1, 90, 2, [10, 100], [(170, 6)]).topics[0]]
        return dict(ots=ots, restarts=4, rhos=(0, 3), prices=_prices(ots, 23), rf3=False)
    if name == "wide":         # 512 replica slots or more: several tournament slots per lane, one scan slot, windowed EXCHANGE above 512 partitions
        ots = [mk("p600", 80, 8, 1, 600, 3, [3, 50], [(80, 1), (81, 4)]).topics[0]]
        return dict(ots=ots, restarts=4, rhos=(0, 3), rf3=True)
    if name == "wide_generic":
        ots = [mk("p300rf2", 70, 5, 1, 300, 2, [9, 33], [(70, 2)]).topics[0]]
        return dict(ots=ots, restarts=4, rhos=(0, 3), rf3=False)
    if name == "curg":         # working words in LDS, current assignment in global memory
        P = 5000
        return dict(ots=_synthetic(ko, 500, 10, P, 3, [], [], 1), restarts=4, rhos=(0, 3), rf3=False,
                    check=lambda st: 16 * P <= st["lds_bytes_search"] < 32 * P)
    if name == "global":       # topic in global memory, one wavefront per restart
        return dict(ots=_synthetic(ko, 1000, 20, 6000, 3, [7, 77, 777], [(1000, 7), (1001, 17), (1002, 17)], 3), restarts=3, rhos=(0, 2),
                    team=1, env={"KAO_CUR_GLOBAL": "0"}, rf3=False, check=lambda st: st["lds_bytes_search"] < 40 * 1024)
    if name == "team":         # a team of four wavefronts on one restart
        return dict(_case(ko, "global"), team=4, env={})
    if name == "one_partition":   # no EXCHANGE partner: every EXCHANGE iteration is skipped
        return dict(ots=[mk("onep", 24, 4, 1, 1, 3, [0], [(24, 1)]).topics[0]], restarts=4, rhos=(0, 1, 3), rf3=True)
    if name == "rf1":             # no LEADER-SWAP candidate: every LEADER-SWAP iteration is skipped
        return dict(ots=[mk("rf1", 30, 3, 1, 40, 1, [2, 11], [(30, 0)]).topics[0]], restarts=4, rhos=(0, 1, 3), rf3=False)
    raise KeyError(name)


CASES = ["rf3", "rf3_generic", "rf2", "rf4", "rf5", "priced", "wide", "wide_generic", "curg", "global", "team", "one_partition", "rf1"]


def _replay(kp, case, seed, iters):
    """The scalar restatement of every (topic, restart) of the case: three launches of `iters` iterations."""
    out = {}
    for ti, ot in enumerate(case["ots"]):
        for rho in case["rhos"]:
            run = kp.PortRun(ot, _tseed(seed, ti), rho, team=max(1, case.get("team", 0)))
            for ln in range(LAUNCHES):
                run.launch(ln, iters, prices=None if case.get("prices") is None else case["prices"][ti])
            out[(ti, rho)] = run.read()
            run.close()
    return out


def _seed(name, iters):
    return 0x51D5 + 131 * CASES.index(name) + iters


@pytest.mark.parametrize("name", CASES)
def test_restatement_accepts_moves_and_does_not_drift(ko, kp, name):
    """CPU half: on every topic of the case the restatement accepts moves at each of the three launch lengths, and its incremental
    V / objective are those of a from-scratch evaluation of the state it ends in."""
    case = _case(ko, name)
    for iters in ITERS:
        refs = _replay(kp, case, _seed(name, iters), iters)
        for ti, ot in enumerate(case["ots"]):
            accepted = [refs[(ti, rho)]["n_accept"] for rho in case["rhos"]]
            print(name, ot.name, "iters", iters, "accepted per restart", accepted)
            assert min(accepted) > 0, (name, ot.name, iters, accepted)
            assert max(accepted) <= LAUNCHES * iters * max(1, case.get("team", 0))
            for rho in case["rhos"]:
                ref = refs[(ti, rho)]
                obj, viol = kp.port_eval(ot, ref["final"])
                assert (obj, int(viol[0])) == (ref["obj"], ref["V"]), (name, ot.name, iters, rho)


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("name", CASES)
def test_kinds_replay_bit_exact(kao, ko, kp, monkeypatch, name, iters):
    """GPU half: three launches of 5, 11 or 19 iterations against the restatement, through the instantiation the case names."""
    case = _case(ko, name)
    for var in ("KAO_SEARCH_RFT", "KAO_CUR_GLOBAL"):
        monkeypatch.delenv(var, raising=False)
    for var, val in case.get("env", {}).items():
        monkeypatch.setenv(var, val)
    seed = _seed(name, iters)
    opts = dict(seed=seed, restarts=case["restarts"], iters_per_launch=iters)
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
        if "check" in case:
            assert case["check"](st), st
        devs = {key: s.restart_state(*key) for key in ((ti, rho) for ti in range(len(case["ots"])) for rho in case["rhos"])}
    refs = _replay(kp, case, seed, iters)
    accepted = 0
    for key, dev in devs.items():
        ref = refs[key]
        assert dev["final"].tolist() == ref["final"].tolist(), (name, iters, key)
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (name, iters, key)
        if ref["best_obj"] >= 0:
            assert dev["best"].tolist() == ref["best"].tolist(), (name, iters, key)
        accepted += ref["n_accept"]
    assert accepted > 0
