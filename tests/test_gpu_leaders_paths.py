"""kao_balance_leaders on the MI355X on both sides of its node threshold: B + 1 <= 2,048 nodes run in the
single workgroup, one more broker in the per-round launches, whose rounds the host settles in batches of eight.  chain(L) of
tests/leaders_ref.py is one phase whose first quiet round is the last of a batch or the first of the next; rows and counters equal
the host model of the kernels, and in the per-round regime the launch count equals what the entry point's schedule gives for the
model's rounds.  tests/test_flow_paths_ref.py holds the chains against HiGHS and their round counts."""
import numpy as np
import pytest

import leaders_ref as lr

pytestmark = pytest.mark.gpu
STAT_CHECKED = [0, 1, 2, 3, 4, 5, 7]   # everything but the launches, which depend on the regime


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _held(kao, rows, B, lo, hi):
    """(result, model's feasible, the model's rounds per phase): status, rows, n_changed and STAT_CHECKED equal the model's."""
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders
    t = Topic(name="t", broker_ids=np.arange(B), rack_of=np.arange(B) % 2, n_racks=2, n_partitions=rows.shape[0], rf=rows.shape[1],
              current=rows.astype(np.uint16), bounds_override={"lead_lo": lo, "lead_hi": hi})
    per_phase = []
    ok, out, n, stats = lr.kernel_model(rows, B, lo, hi, per_phase)
    res = balance_leaders(t)
    print(f"B={B} P={len(rows)} band=[{lo}, {hi}] status={res.status} n_changed={res.n_changed} stats={res.stats.tolist()} model={stats}")
    assert res.status == ("OPTIMAL_PROVEN" if ok else "INFEASIBLE_PROVEN") and res.n_changed == n
    assert (res.assignment.astype(np.int64) == out).all()
    assert [int(res.stats[i]) for i in STAT_CHECKED] == [stats[i] for i in STAT_CHECKED]
    return res, ok, per_phase


@pytest.mark.parametrize("B", [2047, 2048])
@pytest.mark.parametrize("L,rounds", [(6, 8), (7, 9), (14, 16), (15, 17)])
def test_chain_on_both_sides_of_the_node_threshold(kao, L, rounds, B):
    res, ok, per_phase = _held(kao, *lr.chain(L, B))
    assert ok and per_phase == [rounds] and res.n_changed == L
    if B == 2047:
        assert res.stats[6] == 1   # one workgroup ran the whole solve
    else:   # count, start | seed, the batches, pred, extract | apply
        assert res.stats[6] == lr.launches(per_phase, ok) == 6 + 8 * -(-rounds // 8)


def test_band_that_idle_brokers_cannot_meet(kao):
    """chain(7) among 2,048 brokers with lead_lo = 1: broker 7 is served, the 2,040 idle brokers cannot be."""
    res, ok, per_phase = _held(kao, *lr.chain(7, 2048, lo=1))
    assert not ok and res.status == "INFEASIBLE_PROVEN" and res.stats[7] == 2040
    assert res.stats[6] == lr.launches(per_phase, ok)
