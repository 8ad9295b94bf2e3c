"""The RF-3 instantiation of k_search.  A launch group whose topics all have RF 3 and at most 3 current replicas per partition
(LDS-resident, unpriced) runs a kernel whose move arithmetic visits words 0..2 of a partition only: word 3 of the working and the
current words is always the empty word there, which matches no broker and no rack.  It must replay the scalar restatement
(oracle/kao_port.c) bit for bit and leave exactly the state the generic kernel (KAO_SEARCH_RFT=0) leaves.  RF 3 with four
current replicas (an RF decrease: word 3 of the current words is a real replica) and groups that mix RFs keep the generic kernel;
the session statistic `search_rf3_launches` says which one ran."""
import numpy as np
import pytest

from conftest import to_product_topic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _tseed(seed, ti):
    return seed ^ (((ti + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def _run(kao, ots, seed, restarts, launches, iters, rhos, **opts):
    """Device states of restarts `rhos` after `launches` launches, the best keys and the session statistics."""
    with kao.Session([to_product_topic(t) for t in ots], seed=seed, restarts=restarts, iters_per_launch=iters, **opts) as s:
        s.step(launches)
        st = s.stats()
        assert st["drift"] == 0
        states = {(ti, rho): s.restart_state(ti, rho) for ti in range(len(ots)) for rho in rhos}
        return states, s.best_keys().tolist(), st


def _check_replay(kp, ots, seed, launches, iters, states):
    for (ti, rho), dev in states.items():
        ot = ots[ti]
        ref = kp.port_search(ot, _tseed(seed, ti), rho, launches, iters)
        assert dev["final"].tolist() == ref["final"].tolist(), (ot.name, rho)
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == \
               (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (ot.name, rho)
        if ref["best_obj"] >= 0:
            assert dev["best"].tolist() == ref["best"].tolist(), (ot.name, rho)


def _same_states(a, b):
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        assert x["final"].tobytes() == y["final"].tobytes(), key
        assert x["best"].tobytes() == y["best"].tobytes(), key
        assert (x["best_obj"], x["V"], x["obj"], x["n_accept"]) == (y["best_obj"], y["V"], y["obj"], y["n_accept"]), key


def _rf3_topics(ko, weights):
    mk = ko.make_cluster
    return [   # removed brokers leave holes in the current assignment; few partitions make both scan slots share brokers
        mk("h12", 12, 3, 1, 4, 3, [2], [(12, 2)], weights=weights).topics[0],
        mk("h40", 40, 4, 1, 30, 3, [1, 7, 13], [(40, 2), (41, 3)], weights=weights).topics[0],
        mk("h130", 130, 5, 1, 50, 3, [7, 44], [(130, 2)], weights=weights).topics[0],
        mk("uneven", 40, 4, 1, 65, 3, [0, 4, 8, 12, 16, 1], [], weights=weights).topics[0],
        mk("racks100", 300, 100, 1, 120, 3, [1, 2, 3], [(300, 1), (301, 2), (302, 3)], weights=weights).topics[0],
    ]


@pytest.mark.parametrize("weights", [None, ((1, 1), (1, 1)), ((0, 0), (0, 0))], ids=["default", "flat", "zero"])
@pytest.mark.parametrize("wide", [False, True], ids=["small", "wide"])
def test_rf3_kernel_replays_and_matches_generic(kao, ko, kp, monkeypatch, weights, wide):
    """Holes, ties (flat / zero weights: equal costs are the common case), both kWide forms; the fused two-slot REPLACE scan.
    Same sessions with KAO_SEARCH_RFT=0: byte-identical restart states and best keys."""
    kw = {} if weights is None else {"weights": weights}
    ots = _rf3_topics(ko, kw.get("weights", ko.DEFAULT_WEIGHTS))
    if wide:   # 1,500 replica slots: the group's tournament scores several slots per lane
        ots.append(ko.make_cluster("t500", 500, 10, 1, 500, 3, [3, 250], [(500, 1), (501, 4)], **kw).topics[0])
    seed, launches, iters, rhos = 0x5F3A, 2, 256, (0, 2, 5, 7)
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    states, keys, st = _run(kao, ots, seed, 8, launches, iters, rhos)
    assert st["search_rf3_launches"] == launches * st["launch_groups"]
    _check_replay(kp, ots, seed, launches, iters, states)
    monkeypatch.setenv("KAO_SEARCH_RFT", "0")
    states0, keys0, st0 = _run(kao, ots, seed, 8, launches, iters, rhos)
    assert st0["search_rf3_launches"] == 0
    _same_states(states, states0)
    assert keys == keys0


def _drifted(ko, cfg, n):
    from kafka_assignment_optimizer_amd import synthetic
    return [ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                     n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights,
                     bounds_override=dict(pt.bounds_override))
            for pt in synthetic.drift(synthetic.make_config(cfg, n_topics=n), 0.2, 1)]


def test_rf3_elite_reseed_replays(kao, ko, kp, monkeypatch):
    """Elite launches re-seed trailing restarts from the topic's best assignment (the benchmark's topics: config 4, RF 3)."""
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    ots = _drifted(ko, 4, 3)
    assert all(t.rf == 3 and t.current.shape[1] == 3 for t in ots)
    seed, iters = 4243, 120
    with kao.Session([to_product_topic(t) for t in ots], seed=seed, restarts=16, iters_per_launch=iters, elite_period=2) as s:
        s.step(2)
        res = s.best()
        s.step(1)
        st = s.stats()
        assert st["drift"] == 0 and st["search_rf3_launches"] == 3 * st["launch_groups"]
        reseeded = 0
        for ti, ot in enumerate(ots):
            r = res[ti]
            assert r.status != "NO_FEASIBLE"
            for rho in range(16):
                run = kp.PortRun(ot, _tseed(seed, ti), rho)
                run.launch(0, iters)
                run.launch(1, iters)
                before = run.read()
                run.launch(2, iters, elite=(r.assignment, r.objective, r.best_restart))
                ref = run.read()
                dev = s.restart_state(ti, rho)
                assert dev["final"].tolist() == ref["final"].tolist(), (ti, rho)
                assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == \
                       (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (ti, rho)
                reseeded += before["best_obj"] < r.objective and ref["best_obj"] >= r.objective
        assert reseeded > 0


def test_generic_kernel_for_four_current_replicas_and_mixed_rf(kao, ko, kp, monkeypatch):
    """RF 3 with four current replicas per partition (an RF decrease), and one launch group that mixes RF 2 and RF 3: the
    generic kernel runs, and the replays hold."""
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    mk = ko.make_cluster
    seed, launches, iters, rhos = 0x4D3, 2, 128, (0, 3)
    dec = [mk("rf4to3", 40, 4, 1, 30, 4, [3], [(40, 1)], new_rf=3).topics[0]]
    assert dec[0].current.shape[1] == 4
    states, _, st = _run(kao, dec, seed, 4, launches, iters, rhos)
    assert st["search_rf3_launches"] == 0
    _check_replay(kp, dec, seed, launches, iters, states)
    mixed = [mk("rf3", 40, 4, 1, 30, 3, [3], [(40, 1)]).topics[0], mk("rf2", 40, 4, 1, 30, 2, [5], [(40, 2)]).topics[0]]
    states, _, st = _run(kao, mixed, seed, 4, launches, iters, rhos)
    assert st["launch_groups"] == 1 and st["search_rf3_launches"] == 0
    _check_replay(kp, mixed, seed, launches, iters, states)
