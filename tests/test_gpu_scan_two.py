"""The fused two-slot REPLACE scan of k_search (round 7): on LDS-resident, unpriced topics both tournament slots of a scan iteration
are scored in ONE pass over the brokers -- each slot with its own half of the rack table, its own no-candidate bit in the band
state, its own weighted rounds and its own draws (slot 2's by a jump-ahead of the generator).  The moves must be those of the
slot-by-slot scan of the scalar restatement (oracle/kao_port.c) bit for bit.  The shapes below are the ones the fused pass treats
specially."""
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


def _replay(kao, kp, ots, seed, restarts, launches, iters, rhos, prices=None):
    with kao.Session([to_product_topic(t) for t in ots], seed=seed, restarts=restarts, iters_per_launch=iters) as s:
        if prices is not None:
            for ti, pr in enumerate(prices):
                s.set_prices(ti, *pr)
        s.step(launches)
        assert s.stats()["drift"] == 0
        for ti, ot in enumerate(ots):
            for rho in rhos:
                dev = s.restart_state(ti, rho)
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


def _shapes(ko):
    mk = ko.make_cluster
    return [
        # few partitions: the two slots often sit in the same partition, or in partitions that share brokers
        mk("p4", 12, 3, 1, 4, 3, [2], [(12, 2)]).topics[0],
        mk("p6rf4", 9, 3, 1, 6, 4, [0, 5], []).topics[0],
        # every broker in one round (B <= 64): the displaced current replicas of both slots fall into the same weighted round
        mk("b40", 40, 4, 1, 30, 3, [1, 7, 13], [(40, 2), (41, 3)]).topics[0],
        # two and three rounds: weighted rounds of the two slots coincide or are adjacent
        mk("b100", 100, 5, 1, 60, 3, [3, 50, 97], [(100, 0), (101, 4)]).topics[0],
        mk("b170", 170, 7, 1, 90, 2, [10, 100], [(170, 6)]).topics[0],
        # Bx not a multiple of 128 (uneven racks: padding slots inside the index space), RF 1 and an RF change
        mk("uneven", 75, 4, 1, 50, 3, [0, 4, 8, 12, 16, 1], []).topics[0],
        mk("rf1", 30, 2, 1, 20, 1, [3], [(30, 0)]).topics[0],
        mk("rf2to3", 70, 5, 1, 40, 2, [5], [(70, 1), (71, 1), (72, 1)], new_rf=3).topics[0],
        # more racks than lanes: the packed rack table is built in two strides
        mk("racks100", 300, 100, 1, 80, 3, [1, 2, 3], [(300, 1), (301, 2)]).topics[0],
    ]


def test_fused_scan_replay_shapes(kao, ko, kp):
    """Small and odd shapes, several launches: same final state, best snapshot and counters as the slot-by-slot replay."""
    _replay(kao, kp, _shapes(ko), 0x5CA2, restarts=8, launches=3, iters=128, rhos=(0, 1, 4, 7))


def test_fused_scan_replay_long_chain(kao, ko, kp):
    """One small topic, many iterations: the generator state after a fused pass (2 n_rd draws) is what every later draw starts from."""
    ot = ko.make_cluster("chain", 130, 5, 1, 25, 3, [7, 44], [(130, 2)]).topics[0]
    _replay(kao, kp, [ot], 0xC4A1, restarts=4, launches=2, iters=600, rhos=(0, 1, 2, 3))


def test_priced_scan_replay_shapes(kao, ko, kp):
    """The priced instantiation keeps the slot-by-slot scan: replayed with host-set prices on the same shapes."""
    ots = _shapes(ko)[2:6]
    rng = np.random.default_rng(11)
    prices = [(rng.integers(-8, 9, t.n_brokers).astype(np.int32) * 16384, rng.integers(-4, 5, t.n_brokers).astype(np.int32) * 16384,
               rng.integers(-2, 3, t.n_racks).astype(np.int32) * 16384) for t in ots]
    _replay(kao, kp, ots, 0x9A1C, restarts=4, launches=2, iters=128, rhos=(0, 3), prices=prices)


@pytest.mark.parametrize("P", [8192, 8193])
def test_scan_two_limit(kao, ko, kp, P):
    """Topics of exactly kScanTwoSlots (24,576) replica slots scan two slots per iteration (fused), one slot more scans one."""
    from kafka_assignment_optimizer_amd import synthetic as sy
    pt = sy.drift(sy.make_cluster(300, 6, 1, P, 3, [], []), 0.2, 1)[0]
    ot = ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                  n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights)
    _replay(kao, kp, [ot], 0x2457 + P, restarts=2, launches=1, iters=160, rhos=(0, 1))
