"""kao_balance_leaders_cluster on the MI355X against the host model of its kernels (tests/cluster_leaders_ref.py kernel_model), bit
for bit: WHICH of the optimal leader choices it returns, its numbers and its counters (the lowest tight arc
id becomes the predecessor, the marked nodes and then the sink's tight brokers are served in index order with the marks of the
phase's start, rounds are counted up to and including the first quiet one), and on the chains the launch count, which pins the
batches of settle_rounds.  The instances sit on both sides of the dispatch edges of the kernels (tests/test_flow_paths_ref.py
checks that they do, and the model against HiGHS)."""
import numpy as np
import pytest

import cluster_leaders_ref as cr

pytestmark = pytest.mark.gpu
STAT_CHECKED = [0, 1, 2, 3, 4, 6, 7]   # everything but the launches, which launches() states where a test pins them


@pytest.fixture(scope="module")
def call():
    import kafka_assignment_optimizer_amd as k
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_cluster_arrays
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return balance_leaders_cluster_arrays


def _held(call, rows, topic_of, B, LO, tlo, thi, cluster_hi=-1):
    """One instance through the GPU: status, rows, n_changed, both peaks and stats[0..4, 6, 7] equal the model's; a dry run reports
    the same numbers on untouched rows.  Returns (result, model result, the model's solves)."""
    rows = np.asarray(rows, dtype=np.int64)
    solves = []
    model = cr.kernel_model(rows, topic_of, B, LO, tlo, thi, cluster_hi, solves=solves)
    ok, out, n, before, after, stats = model
    res = call(rows, B, topic_of, tlo, thi, LO, cluster_hi)
    dry = call(rows, B, topic_of, tlo, thi, LO, cluster_hi, dry_run=True)
    print(f"B={B} P={len(rows)} lo={LO} hi={cluster_hi} gpu={res.status, res.n_changed, res.peak_before, res.peak_after} "
          f"stats={res.stats.tolist()} model={n, before, after} {stats}")
    assert res.status == ("OPTIMAL_PROVEN" if ok else "INFEASIBLE_PROVEN")
    assert (res.n_changed, res.peak_before, res.peak_after) == (n, before, after)
    assert (res.rows.astype(np.int64) == out).all(), np.nonzero((res.rows != out).any(axis=1))[0][:10]
    assert res.stats[STAT_CHECKED].tolist() == [stats[i] for i in STAT_CHECKED]
    assert (dry.rows == rows).all() and (dry.status, dry.n_changed, dry.peak_before, dry.peak_after) == (res.status, n, before, after)
    assert dry.stats.tolist() == res.stats.tolist()
    return res, model, solves


def test_small_family_equals_the_model(call):
    """All 80 seeds of small_case without a cap and, where that is feasible, at a cap one above and one below the optimum."""
    runs = infeasible = 0
    for seed in range(80):
        case = cr.small_case(seed)
        _, model, _ = _held(call, *case)
        runs += 1
        infeasible += not model[0]
        if model[0]:
            peak = model[4]
            _held(call, *case, cluster_hi=peak + 1)
            runs += 1
            if peak - 1 >= case[3]:   # (a cap below cluster_lo is an invalid argument)
                res, _, _ = _held(call, *case, cluster_hi=peak - 1)
                assert res.status == "INFEASIBLE_PROVEN" and res.stats[7] > 0
                runs += 1
    assert runs >= 180 and 5 <= infeasible <= 30, (runs, infeasible)


def test_mid_instance_equals_the_model(call):
    rows, topic_of = cr.mid_case(100, 20, 150, 3, 0)
    res, _, _ = _held(call, rows, topic_of, 100, 0, np.zeros(20, dtype=np.int64), np.full(20, 3))
    assert (res.peak_before, res.peak_after, res.n_changed) == (75, 30, 406)


@pytest.mark.parametrize("L,rounds", [(4, 8), (5, 9), (12, 16), (13, 17)])
def test_settle_batch_edge(call, L, rounds):
    """chain(L): one phase whose first quiet round is the last of a batch of eight (8, 16) or the first of the next (9, 17).  The
    launch count says how many batches were enqueued, the round count where the host stopped counting."""
    res, model, solves = _held(call, *cr.chain(L))
    assert [s["rounds"] for s in solves] == [[rounds]] and res.stats[2] == rounds
    assert res.stats[5] == cr.launches(L + 1, solves, model[0]) == 9 + 8 * -(-rounds // 8)


def test_lead_is_reset_beyond_the_first_block(call):
    """P = 257 > 256 >= Q = 4 (the grid of k_lc_start_pairs comes from P): row 256 moves in infeasible probes and must start the next
    solve from slot 0 again."""
    res, model, solves = _held(call, *cr.probes_case())
    assert res.stats[0] == len(solves) >= 4 and (res.peak_after, res.n_changed) == (101, 3)
    assert res.stats[5] == cr.launches(257, solves, True)


def test_more_nodes_than_slots(call):
    """600 brokers with chain(5) among them: N = 607 > PW = 12 (the grid of the rounds comes from N)."""
    res, model, solves = _held(call, *cr.wide_index_case())
    assert res.stats[5] == cr.launches(6, solves, True)


@pytest.mark.parametrize("extra", [0, 1])
def test_mark_ballot_edge(call, extra):
    """cluster_lo = 1 with deficit broker nodes up to T - 1: T = 64 (one full ballot, its last lane a deficit node) and T = 65
    (deficit nodes at 63, and at 64 alone in the second ballot).  deficit_case asserts the indices."""
    res, _, _ = _held(call, *cr.deficit_case(extra))
    assert res.status == "OPTIMAL_PROVEN" and res.n_changed == 16


def test_width_8_with_padding(call):
    res, _, _ = _held(call, *cr.width8_case())
    assert res.status == "OPTIMAL_PROVEN" and res.n_changed > 0
