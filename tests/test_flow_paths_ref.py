"""The instances that sit on the dispatch edges of kao_failover_order, kao_failover_order_weighted, kao_balance_leaders_cluster and
kao_balance_leaders (DESIGN.md sections 4h, 4i, 4j, 4l), checked from the references alone: every builder meets the conditions it
was built for, the host models of the kernels (`kernel_model` of failover_ref, cluster_leaders_ref, leaders_ref) agree with HiGHS on
all of them, and their counters and launch counts equal vectors worked out by hand.  tests/test_gpu_failover_paths.py,
tests/test_gpu_cluster_leaders_paths.py, tests/test_gpu_leaders_paths.py and tests/test_gpu_wfailover.py hold the GPU to these
models bit for bit."""
import numpy as np
import pytest

import cluster_leaders_ref as cr
import failover_ref as fr
import leaders_ref as lr


# ---- kao_failover_order ---------------------------------------------------------------------------------------------------------------
def failover_cases():
    """(name, rows, B, rack_of, R, scope) of every edge case of tests/test_gpu_failover_paths.py that runs in the test's process."""
    out = []
    for n in (256, 257):
        out += [(f"hot{n}", *fr.hot_leader_instance(n), scope) for scope in (0, 1)]
    for B in (64, 65):
        out += [(f"bitmap{B}", *fr.bitmap_instance(B), scope) for scope in (0, 1)]
    for B in (1024, 1025):
        out.append((f"offsets{B}", *fr.limit_instance(B), 0))
    return out


@pytest.mark.parametrize("case", failover_cases(), ids=lambda c: f"{c[0]}-scope{c[5]}")
def test_failover_model_matches_highs(case):
    _, rows, B, rack_of, R, scope = case
    after, scen, stats = fr.kernel_model(rows, B, rack_of, scope, R, with_stats=True)
    opt = fr.scenario_optimum(rows, B, rack_of, scope, R)
    assert (scen == opt).all()
    assert fr.check_rows(rows, after, B, rack_of, scope) == int(opt[:, 4].sum())
    assert stats[0] == int((opt[:, 0] > 0).sum()) and stats[1] >= stats[0] and stats[4] >= int((opt[:, 2] - opt[:, 3]).max())


@pytest.mark.parametrize("B", [3048, 3049])
def test_failover_lds_limit_instances_match_highs(B):
    rows, B, rack_of, R = fr.limit_instance(B)
    after, scen, stats = fr.kernel_model(rows, B, rack_of, 0, R, with_stats=True)
    assert (scen == fr.scenario_optimum(rows, B, rack_of, 0, R)).all()
    assert stats[0] == 40 and int(scen[:, 4].sum()) == 57 and scen[B - 1, 0] > 0


def test_failover_edges_sit_where_the_kernels_decide():
    # lanes per workgroup: at most 1,024 slots in the largest scenario keep 256 lanes
    assert [fr.largest_slots(*fr.hot_leader_instance(n)[:3], 0, 5) for n in (256, 257)] == [1024, 1028]
    # dynamic LDS against what a launch may ask for unopened: 48 KiB (kao_failover_order), 32 KiB (kao_failover_order_weighted)
    assert [fr.lds_bytes(B) for B in (3048, 3049)] == [49152, 49168] and 49152 == 48 * 1024
    assert [fr.weighted_lds_bytes(B) for B in (2048, 2049)] == [32768, 32784] and 32768 == 32 * 1024
    # k_fo_offsets: one workgroup of 1,024 lanes takes ceil(G / 1024) scenarios per lane
    assert [-(-fr.n_scenarios(B, None, 0) // 1024) for B in (1024, 1025)] == [1, 2]
    for B in (1024, 1025, 2048, 2049, 3048, 3049):   # the last broker is in use: the last scenario has work
        rows = fr.limit_instance(B)[0]
        assert (rows[:, 0] == B - 1).any() and len(np.unique(rows)) == 40
    # bitmap words: B % 32 in {0, 1}; bitmap_instance itself asserts the targets 31, 32 and B - 1 from the model's phases
    assert [B % 32 for B in (64, 65)] == [0, 1] and [(B + 31) // 32 for B in (64, 65)] == [2, 3]


def test_failover_stats_by_hand():
    """two_arc_instance in broker scope.  Scenario 0: bisection between 2 and 3, the probe at 2 and the final solve at 2 each run one
    phase of three rounds (two arcs, then the quiet round) and one path of two arcs.  Scenarios 1 and 2 (one affected partition with
    one eligible slot): the probe at 3 runs one phase of one quiet round and proves it infeasible, the final solve at 4 has no excess.
    Broker 3 leads nothing: no scenario."""
    rows, B, rack_of, R = fr.two_arc_instance()
    after, scen, stats = fr.kernel_model(rows, B, rack_of, 0, R, with_stats=True)
    assert stats == [3, 2 + 2 + 2, 2 + 1 + 1, 6 + 1 + 1, 2, 2]
    plain = fr.kernel_model(rows, B, rack_of, 0, R)
    assert len(plain) == 2 and (plain[0] == after).all() and (plain[1] == scen).all()
    # nothing affected anywhere: no scenario counts, no probe
    assert fr.kernel_model(np.array([[0], [1]]), 3, np.arange(3), 0, 3, with_stats=True)[2] == [0] * 6
    # RF 2: one eligible slot each, nothing to choose.  Brokers 0 and 1 lead one partition each and inherit the other's.
    _, scen, stats = fr.kernel_model(np.array([[0, 1], [1, 0]]), 2, np.arange(2), 0, 2, with_stats=True)
    assert scen.tolist() == [[1, 0, 2, 2, 0]] * 2 and stats == [2, 2, 0, 0, 0, 0]   # lo == hi: only the final solve, without excess


# ---- kao_balance_leaders_cluster ------------------------------------------------------------------------------------------------------
def cluster_cases():
    """(name, rows, topic_of, B, cluster_lo, tlo, thi, cluster_hi) of every edge case of tests/test_gpu_cluster_leaders_paths.py."""
    out = [(f"chain{L}", *cr.chain(L)) for L in (4, 5, 12, 13)]
    out.append(("probes", *cr.probes_case(), -1))
    out.append(("wide_index", *cr.wide_index_case()))
    out += [(f"deficit{extra}", *cr.deficit_case(extra), -1) for extra in (0, 1)]
    out.append(("width8", *cr.width8_case(), -1))
    return out


@pytest.mark.parametrize("case", cluster_cases(), ids=lambda c: c[0])
def test_cluster_model_matches_highs(case):
    _, rows, topic_of, B, LO, tlo, thi, chi = case
    ok, out, n, before, after, stats = cr.kernel_model(rows, topic_of, B, LO, tlo, thi, chi)
    assert ok and cr.check_rows(rows, out) == n
    if chi < 0:
        assert (after, n) == cr.optimum(rows, topic_of, B, LO, tlo, thi)
    else:
        assert n == cr.lp(rows, topic_of, B, LO, chi, tlo, thi) and after <= chi
    assert cr.admissible(out, topic_of, B, LO, after, tlo, thi)


def test_cluster_edges_sit_where_the_kernels_decide():
    # settle_rounds reads the flags every 8 rounds: the quiet round is the last of a batch, or the first of the next
    for L, rounds in ((4, 8), (5, 9), (12, 16), (13, 17)):
        solves = []
        cr.kernel_model(*cr.chain(L), solves=solves)
        assert [s["rounds"] for s in solves] == [[rounds]]
    # grids: sblocks = grid_for(max(P, Q)) with P > 256 >= Q, ablocks = grid_for(max(PW, N)) with N > PW
    rows, topic_of, B, LO, tlo, thi = cr.probes_case()
    net = cr._Net(rows, topic_of, B, tlo, thi)
    assert net.P > 256 >= net.Q == 4
    rows, topic_of, B, LO, tlo, thi, chi = cr.wide_index_case()
    net = cr._Net(rows, topic_of, B, tlo, thi)
    assert net.N == 607 > rows.size == 12 and net.N > 2 * 256   # more than two blocks of nodes
    # (deficit_case asserts its node indices against the 64-wide ballots itself)
    rows = cr.width8_case()[0]
    assert rows.shape[1] == 8 and (rows == cr.NONE).any()


def test_cluster_stats_and_launches_by_hand():
    """chain(5): broker 0 has the one unit of excess, the sink the deficit.  The keys reach broker 0's pair, the pairs of brokers 1..5
    over the five partition arcs, broker 5 and the sink in 8 rounds; the ninth changes nothing.  One path of 8 arcs."""
    case = cr.chain(5)
    solves = []
    ok, _, n, before, after, stats = cr.kernel_model(*case, solves=solves)
    assert stats == [1, 1, 9, 1, 8, 0, 6, 0]
    # count + peak | start x 2 | seed, 16 rounds, pred, extract | peak of f | apply
    assert cr.launches(6, solves, ok) == 2 + 2 + (1 + 16 + 2) + 1 + 1
    solves = []
    ok = cr.kernel_model(*cr.chain(4), solves=solves)[0]
    assert cr.launches(5, solves, ok) == 2 + 2 + (1 + 8 + 2) + 1 + 1
    # no partition: the peak of the input; the probe without a cap and the final solve, each without a phase, and their peaks;
    # nothing to apply
    solves = []
    ok = cr.kernel_model(np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64), 4, 0, [0], [1], solves=solves)[0]
    assert ok and cr.launches(0, solves, ok) == 1 + (2 + 1) + (2 + 1)
    # an infeasible solve has no peak to take and nothing to apply: [[0], [0]] with the band [0, 1] on one topic
    solves = []
    ok = cr.kernel_model(np.array([[0], [0]]), np.array([0, 0]), 2, 0, [0], [1], solves=solves)[0]
    assert not ok and [s["rounds"] for s in solves] == [[1]] and cr.launches(2, solves, ok) == 2 + 2 + (1 + 8 + 2)


# ---- kao_balance_leaders --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2047, 2048])
@pytest.mark.parametrize("L", [6, 7, 14, 15])
def test_leaders_chain_matches_highs_and_its_rounds(L, B):
    rows, B, lo, hi = lr.chain(L, B)
    per_phase = []
    ok, out, n, stats = lr.kernel_model(rows, B, lo, hi, per_phase)
    assert ok and n == lr.lp_optimum(rows, B, lo, hi) == L and lr.check_swap(rows, out) == n
    assert per_phase == [{6: 8, 7: 9, 14: 16, 15: 17}[L]]
    assert (B + 1 <= 2048) == (B == 2047)   # kLeadSoloNodes: B = 2047 runs in one workgroup, B = 2048 in per-round launches


def test_leaders_stats_and_launches_by_hand():
    """chain(6, 7): broker 0 has the excess, the sink the deficit; six partition arcs and broker 6's arc into the sink settle in 7
    rounds, the eighth changes nothing; one path of 7 arcs; one partition over the band, none under it."""
    per_phase = []
    ok, _, n, stats = lr.kernel_model(*lr.chain(6, 7), per_phase)
    assert stats == [1, 8, 1, 7, 1, 0, 0, 0]
    assert lr.launches(per_phase, ok) == 2 + (1 + 8 + 2) + 1   # count, start | seed, 8 rounds, pred, extract | apply
    ok = lr.kernel_model(*lr.chain(7, 8), per_phase)[0]
    assert lr.launches(per_phase, ok) == 2 + (1 + 16 + 2) + 1
    # lead_lo = 1 with idle brokers: broker 7 is served over the chain (8 rounds: it is a deficit node itself), the 2,040 idle
    # brokers cannot be; the second phase's one round finds no excess left to start from.  No apply.
    rows, B, lo, hi = lr.chain(7, 2048, lo=1)
    ok, out, n, stats = lr.kernel_model(rows, B, lo, hi, per_phase)
    assert not ok and lr.lp_optimum(rows, B, lo, hi) is None and per_phase == [8, 1] and stats[7] == 2040
    assert lr.launches(per_phase, ok) == 2 + (1 + 8 + 2) + (1 + 8 + 2)
