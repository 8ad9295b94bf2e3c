"""kao_plan_waves_headroom on the MI355X, one case per kernel path at its smallest shape: capacities above 2^63 (free bytes are
clamped before they are compared), brokers beyond 256 x the workgroups of an order (the strided row clear of k_head_round, the
per-thread broker loop of k_head_close, the wider grid of k_head_init), ties of the least free bytes within a thread, between
threads and between waves, rows of width 8 with nine participants, without a source, of changing RF, 255 / 256 / 257 moving
partitions, seeds 0, 2^63 and 2^64 - 1, 1,000 moving partitions over four workgroups, and a last order that ends in the last
round of a batch of 32 or in the first of the next.  Every result goes through the _exact of tests/test_gpu_waves_headroom.py:
bit for bit the sequential reference (wave, n_waves, lower_bound, stats[0..3] and [5..7]) and accepted by the independent
checker.  The instances are built in tests/headroom_paths_cases.py and their properties verified on the CPU in
tests/test_waves_headroom_paths_ref.py.

Not covered: fewer than 64 orders.  Per-order state is 60 B + 8 n_mv bytes against a budget of 2^30, and at most 65,534 brokers
can be declared, so the count drops to 63 only above 1,605,000 moving partitions, where the sequential reference cannot run 63
orders in test time.  The order-count rule is covered for the layouts of the older planners by
test_gpu_waves_paths.py::test_order_budget_decides_whether_a_late_winner_runs."""
import pytest

import headroom_paths_cases as hc
from test_gpu_waves_headroom import _exact

pytestmark = pytest.mark.gpu
I64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _same(case):
    _, cur, tgt, size, stored, capacity, C, k, seed = case
    return _exact(cur, tgt, size, stored, capacity, C, k, seed)


def _named(cases, name):
    return next(c for c in cases if c[0] == name)


@pytest.mark.parametrize("name, least", [("clamp/all", [I64_MAX, 0, 1]), ("clamp/control", [(1 << 63) - 115, 0, 2]),
                                         ("clamp/waves", [I64_MAX, 0, 1])])
def test_free_bytes_are_clamped_before_they_are_compared(kao, name, least):
    """Capacity 2^64 - 1: every free value is above 2^63 - 1, so the first wave and the lowest receiving broker are reported,
    not the broker (clamp/all) or the wave (clamp/waves) with the fewest unclamped bytes.  At capacity 2^63 nothing is clamped."""
    assert _same(_named(hc.clamp_cases(), name))[3][5:].tolist() == least


@pytest.mark.parametrize("name", ["wide/1000", "wide/257"])
def test_brokers_beyond_the_threads_of_an_order(kao, name):
    """Five slots, so 256 threads per order, and four arrivals at broker 999 (256) at k = 1: its minimum key is cleared by the
    stride of the row clear, and its arrivals are closed by the stride of k_head_close."""
    wave, nw, _, stats = _same(_named(hc.wide_cases(), name))
    assert (wave.tolist(), nw) == ([0, 1, 2, 3, 0], 4) and stats[7] == int(name.split("/")[1]) - 1


@pytest.mark.parametrize("name, least", [("tie/thread", [40, 0, 44]), ("tie/threads", [40, 0, 45]), ("tie/strict", [39, 0, 999]),
                                         ("tie/waves", [40, 0, 44])])
def test_least_free_ties(kao, name, least):
    """Equal free bytes at two brokers of one thread of k_head_close, of two threads, and of two waves; a strict minimum in a
    thread's last stride."""
    assert _same(_named(hc.tie_cases(), name))[3][5:].tolist() == least


@pytest.mark.parametrize("name", hc.SHAPE_NAMES)
def test_row_shapes_bit_for_bit(kao, name):
    """The sized row shapes of waves_paths_cases with capacity = 100 / 110 / 120 % of the larger of what a broker holds before
    and after the plan: capacity binds on nine-participant rows, on rows without a source and across RF changes."""
    _same(_named(hc.shape_cases(), name))


@pytest.mark.parametrize("name", sorted(hc.MID))
def test_mid_plan_bit_for_bit(kao, name):
    """1,000 moving partitions on 40 brokers: four workgroups per order whose joiners store into one order's loads, dozens of
    waves and hundreds of rounds, the orders at different waves within a launch."""
    _same(hc.mid_case(name))


@pytest.mark.parametrize("i", range(3))
def test_the_last_order_ends_on_either_side_of_a_batch(kao, i):
    """Every order is done in round index 30, 31 (the last of the first batch of 32) and 32 (the first of the second): the round
    counts are derived in headroom_paths_cases.conveyor from the round rules, not read from a device."""
    case, _, launches = hc.conveyor_cases()[i]
    assert _same(case)[3][4] == launches
