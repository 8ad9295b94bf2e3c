"""The paths of k_search's iteration that round 10 restated, replayed bit for bit against the scalar restatement
(oracle/kao_port.c: restart states, best snapshots, objective / violation / accepted-move counters):

- the accepted-move update rebuilds only the band-state row whose count moved (replica row for a follower REPLACE, leader row for
  a LEADER-SWAP or a leader/follower EXCHANGE, both for a leader REPLACE, none for an EXCHANGE between slots of one kind).  A
  wrong row in the band state changes a later scan, so the cases run several launches in a row on drifted topics where all
  four move types are accepted many times, through the RF-3 kernel, the generic one (KAO_SEARCH_RFT=0, byte-identical states),
  eight words per partition (RF 5), and the priced instantiation (which also reads the price flags of the rows);
- the fused two-slot scan runs two plain rounds per trip and marks slot 2's no-candidate brokers in the cost field;
- the EXCHANGE partner round forms the part of the rack delta that does not depend on the partner slot once, and (RF 3) the
  partner partition's per-rack counts from the three pairwise rack equalities: several partner rounds, the windowed form, and
  two racks (many equal racks inside a partition);
- hole filling of the initialising launch: no hole, leader holes only, a partition that lost every replica, and flat / zero
  weights, where ties between brokers are the common case.
Integer replays: nothing is compared with a tolerance."""
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


def _run(kao, ots, seed, restarts, launches, iters, rhos, prices=None):
    with kao.Session([to_product_topic(t) for t in ots], seed=seed, restarts=restarts, iters_per_launch=iters) as s:
        if prices is not None:
            for ti, pr in enumerate(prices):
                s.set_prices(ti, *pr)
        s.step(launches)
        st = s.stats()
        assert st["drift"] == 0
        return {(ti, rho): s.restart_state(ti, rho) for ti in range(len(ots)) for rho in rhos}, s.best_keys().tolist(), st


def _check(kp, ots, seed, launches, iters, states, prices=None):
    accepted = 0
    for (ti, rho), dev in states.items():
        ot = ots[ti]
        if prices is None:
            ref = kp.port_search(ot, _tseed(seed, ti), rho, launches, iters)
        else:
            run = kp.PortRun(ot, _tseed(seed, ti), rho)
            for ln in range(launches):
                run.launch(ln, iters, prices=prices[ti])
            ref = run.read()
            run.close()
        assert dev["final"].tolist() == ref["final"].tolist(), (ot.name, rho)
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == \
               (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (ot.name, rho)
        if ref["best_obj"] >= 0:
            assert dev["best"].tolist() == ref["best"].tolist(), (ot.name, rho)
        accepted += ref["n_accept"]
    return accepted


def _same_states(a, b):
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        assert x["final"].tobytes() == y["final"].tobytes(), key
        assert x["best"].tobytes() == y["best"].tobytes(), key
        assert (x["best_obj"], x["V"], x["obj"], x["n_accept"]) == (y["best_obj"], y["V"], y["obj"], y["n_accept"]), key


def _drifted(ko, cfg, n):
    from kafka_assignment_optimizer_amd import synthetic
    return [ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                     n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights,
                     bounds_override=dict(pt.bounds_override))
            for pt in synthetic.drift(synthetic.make_config(cfg, n_topics=n), 0.2, 1)]


def test_accepted_moves_three_launches_rf3_and_generic(kao, ko, kp, monkeypatch):
    """The benchmark's topics (config 4 after a 20 % drift), three launches in a row: every accepted move's band-state row feeds
    the scans that follow.  RF-3 kernel, then the generic kernel with byte-identical states."""
    ots = _drifted(ko, 4, 3)
    assert all(t.rf == 3 and t.n_partitions == 50 and t.n_brokers == 500 for t in ots)
    seed, launches, iters, rhos = 0xACCE, 3, 256, (0, 1, 3, 6, 9, 15)
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    states, keys, st = _run(kao, ots, seed, 16, launches, iters, rhos)
    assert st["search_rf3_launches"] == launches * st["launch_groups"]
    accepted = _check(kp, ots, seed, launches, iters, states)
    assert accepted > 20 * len(states)   # the update is exercised: many accepted moves per restart
    monkeypatch.setenv("KAO_SEARCH_RFT", "0")
    states0, keys0, st0 = _run(kao, ots, seed, 16, launches, iters, rhos)
    assert st0["search_rf3_launches"] == 0
    _same_states(states, states0)
    assert keys == keys0


@pytest.mark.parametrize("rf", [2, 4, 5])
def test_accepted_moves_other_replication_factors(kao, ko, kp, monkeypatch, rf):
    """RF 2 and RF 4 (four words per partition, generic kernel) and RF 5 (eight words)."""
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    ot = ko.make_cluster("rf%d" % rf, 90, 6, 1, 40, rf, [4, 31, 77], [(90, 1), (91, 5)]).topics[0]
    seed, launches, iters, rhos = 0xF00 + rf, 3, 192, (0, 2, 5)
    states, _, st = _run(kao, [ot], seed, 8, launches, iters, rhos)
    assert st["search_rf3_launches"] == 0
    assert _check(kp, [ot], seed, launches, iters, states) > 0


def test_accepted_moves_priced(kao, ko, kp, monkeypatch):
    """The priced instantiation reads the price flags of both rows of the band state: host-set prices, three launches."""
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    mk = ko.make_cluster
    ots = [mk("b100", 100, 5, 1, 60, 3, [3, 50, 97], [(100, 0), (101, 4)]).topics[0],
           mk("b170", 170, 7, 1, 90, 2, [10, 100], [(170, 6)]).topics[0],
           mk("rf4", 60, 4, 1, 40, 4, [5], [(60, 1)]).topics[0]]
    rng = np.random.default_rng(23)
    prices = [(rng.integers(-8, 9, t.n_brokers).astype(np.int32) * 16384, rng.integers(-4, 5, t.n_brokers).astype(np.int32) * 16384,
               rng.integers(-2, 3, t.n_racks).astype(np.int32) * 16384) for t in ots]
    seed, launches, iters, rhos = 0x9B1C, 3, 128, (0, 3)
    states, _, _ = _run(kao, ots, seed, 4, launches, iters, rhos, prices=prices)
    assert _check(kp, ots, seed, launches, iters, states, prices=prices) > 0


def test_exchange_partner_rounds(kao, ko, kp, monkeypatch):
    """EXCHANGE: more than 64 partitions (several partner rounds), more than 512 (the windowed form), and two racks, where the
    replicas of a partition share racks all the time -- through the RF-3 kernel and the generic one, byte-identical."""
    mk = ko.make_cluster
    ots = [mk("p130", 60, 5, 1, 130, 3, [7, 44], [(60, 2)]).topics[0],
           mk("p600", 80, 8, 1, 600, 3, [3, 50], [(80, 1), (81, 4)]).topics[0],
           mk("racks2", 20, 2, 1, 30, 3, [3], [(20, 1)]).topics[0],
           mk("racks2b", 31, 2, 1, 70, 3, [0, 9], []).topics[0]]
    seed, launches, iters, rhos = 0xE8C4, 2, 256, (0, 1, 4, 7)
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    states, keys, st = _run(kao, ots, seed, 8, launches, iters, rhos)
    assert st["search_rf3_launches"] == launches * st["launch_groups"]
    assert _check(kp, ots, seed, launches, iters, states) > 0
    monkeypatch.setenv("KAO_SEARCH_RFT", "0")
    states0, keys0, st0 = _run(kao, ots, seed, 8, launches, iters, rhos)
    assert st0["search_rf3_launches"] == 0
    _same_states(states, states0)
    assert keys == keys0


def _hole_topics(ko, weights):
    mk = ko.make_cluster
    none = mk("nohole", 40, 4, 1, 30, 3, [], [(40, 1), (41, 2)], weights=weights).topics[0]
    assert not (none.current == ko.NONE).any()
    lead = mk("leadholes", 50, 5, 1, 40, 3, [], [(50, 0)], weights=weights).topics[0]
    lead.current[[1, 8, 9, 22, 39], 0] = ko.NONE   # leaders gone, followers all there
    assert not (lead.current[:, 1:] == ko.NONE).any()
    lost = mk("lostall", 45, 3, 1, 35, 3, [6], [(45, 2)], weights=weights).topics[0]
    lost.current[11, :] = ko.NONE                  # one partition has no surviving replica
    mixed = mk("holes", 130, 5, 1, 50, 3, [7, 44, 90], [(130, 2)], weights=weights).topics[0]
    return [none, lead, lost, mixed]


@pytest.mark.parametrize("weights", [None, ((1, 1), (1, 1)), ((0, 0), (0, 0))], ids=["default", "flat", "zero"])
def test_hole_filling_shapes(kao, ko, kp, monkeypatch, weights):
    """The initialising launch: no hole, leader holes only, a partition that lost all its replicas, ordinary holes; with flat and
    zero weights the tie byte decides most insertions.  One short launch (the fill dominates), then a second one."""
    monkeypatch.delenv("KAO_SEARCH_RFT", raising=False)
    ots = _hole_topics(ko, ko.DEFAULT_WEIGHTS if weights is None else weights)
    for launches, iters in ((1, 8), (2, 160)):
        seed, rhos = 0x401E + launches, (0, 1, 2, 5, 7)
        states, _, _ = _run(kao, ots, seed, 8, launches, iters, rhos)
        _check(kp, ots, seed, launches, iters, states)
