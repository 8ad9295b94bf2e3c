"""Ties in the fused two-slot REPLACE scan of k_search: one wavefront reduction picks both the slot and the lane of the move, over
(key << 7 | slot << 6 | lane).  The rule it must keep is the slot-by-slot one of the scalar restatement (oracle/kao_port.c): the
strictly lower key wins, equal keys go to slot 1, then to the lowest lane.  Flat objective weights make equal costs the common
case, so the 8 tie bits of the draws decide, and often fail to: the replay then checks the slot and lane order bit for bit.
The marks of both slots' brokers in the band state (a broker in both partitions carries both bits) are exercised by topics of
few partitions, where the two slots often share a partition or brokers."""
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


def _replay(kao, kp, ots, seed, restarts, launches, iters, rhos):
    with kao.Session([to_product_topic(t) for t in ots], seed=seed, restarts=restarts, iters_per_launch=iters) as s:
        s.step(launches)
        assert s.stats()["drift"] == 0
        for ti, ot in enumerate(ots):
            for rho in rhos:
                dev = s.restart_state(ti, rho)
                ref = kp.port_search(ot, _tseed(seed, ti), rho, launches, iters)
                assert dev["final"].tolist() == ref["final"].tolist(), (ot.name, rho)
                assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == \
                       (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (ot.name, rho)
                if ref["best_obj"] >= 0:
                    assert dev["best"].tolist() == ref["best"].tolist(), (ot.name, rho)


@pytest.mark.parametrize("weights", [((1, 1), (1, 1)), ((0, 0), (0, 0))], ids=["flat", "zero"])
def test_fused_scan_ties_replay(kao, ko, kp, weights):
    """Flat and zero objective weights: most candidates of both slots share a cost."""
    mk = ko.make_cluster
    ots = [
        mk("t2", 12, 3, 1, 4, 3, [2], [(12, 2)], weights=weights).topics[0],
        mk("t40", 40, 4, 1, 30, 3, [1, 7, 13], [(40, 2), (41, 3)], weights=weights).topics[0],
        mk("t130", 130, 5, 1, 50, 3, [7, 44], [(130, 2)], weights=weights).topics[0],
        mk("t500", 500, 10, 1, 50, 3, [3, 250], [(500, 1), (501, 4)], weights=weights).topics[0],
    ]
    _replay(kao, kp, ots, 0x71E5, restarts=8, launches=2, iters=256, rhos=(0, 2, 5, 7))
