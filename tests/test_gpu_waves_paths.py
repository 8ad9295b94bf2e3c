"""kao_plan_waves and kao_plan_waves_sized on the MI355X, one case per kernel path at its smallest shape: fewer than 64 orders (the
order budget), a first fit that reaches the last wave of the load arrays, a last placement on either side of a batch of 32
rounds, the sized planner over several workgroups and batches, and rows of width 8, without a source, padded with NONE or of
changing RF.  Every result goes through the independent checker and is then compared bit for bit (wave, n_waves, lower_bound)
with the host restatement run with the order count the budget rule gives.  The instances are built and their properties
verified on the CPU in tests/waves_paths_cases.py and tests/test_waves_cap_ref.py.

Not covered: saturation of the key's degree field at 0xFFFF.  It needs 65,536 movements at one broker, where the sequential
reference is quadratic."""
import pytest

import waves_paths_cases as wc
import waves_ref as wr
import waves_sized_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _plan(case, B=None):
    from kafka_assignment_optimizer_amd.waves import plan_waves_arrays, plan_waves_sized_arrays
    _, cur, tgt, size, C, k, seed = case
    B = wc.brokers_of(case) if B is None else B
    if size is None:
        wave, nw, lb = plan_waves_arrays(cur, tgt, B, k, seed)
        wr.check(cur, tgt, k, wave, nw, lb)
    else:
        wave, nw, lb = plan_waves_sized_arrays(cur, tgt, B, size, C, k, seed)
        sr.check_sized(cur, tgt, size, C, k, wave, nw, lb)
    return wave, nw, lb


def _same(case, B=None):
    """Checked result == the model with the order count of (B, wave cap, moving partitions, layout).  Returns the result."""
    wave, nw, lb = _plan(case, B)
    n_ord = wr.order_count(wc.brokers_of(case) if B is None else B, wc.case_cap(case), wc.n_moving(case), case[3] is not None, case[5])
    mwave, mnw, mlb = wc.run_model(case, n_ord)
    assert (nw, lb) == (mnw, mlb), (case[0], n_ord)
    assert wave.tolist() == mwave.tolist(), (case[0], n_ord)
    return wave, nw, lb


@pytest.mark.parametrize("layout", [4, 8, 12])
def test_order_budget_decides_whether_a_late_winner_runs(kao, layout):
    """330 partitions on 12 brokers whose best order is j (42 count-only, 40 sized with k = 0, 20 sized with k = 1), declared
    over so many idle brokers that the per-order state of about 25 / 26 / 51 MB leaves room for j + 1 orders, and over one
    broker more, which leaves room for j: the first result is order j's, the second has one wave more."""
    case, j = wc.budget_case(layout)
    sized, k = case[3] is not None, case[5]
    wcap, n_mv = wc.case_cap(case), wc.n_moving(case)
    b_in = wc.brokers_for(case, j + 1)
    assert wr.order_count(b_in, wcap, n_mv, sized, k) == j + 1 and wr.order_count(b_in + 1, wcap, n_mv, sized, k) == j
    included = _same(case, b_in)[1]
    excluded = _same(case, b_in + 1)[1]
    assert excluded > included
    assert included == wc.run_model(case, 64)[1]     # with room for all 64 the winner is still order j
    assert _same(case)[1] == included                # and the plain index of 12 brokers runs all 64


def test_one_order(kao):
    """The order budget at its floor: 65,534 brokers x a wave cap of 2,062 leave room for one order (516 MiB)."""
    case = wc.one_order_case()
    assert wr.order_count(65534, wc.case_cap(case), wc.n_moving(case), False, 1) == 1
    assert _same(case, 65534)[1:] == (230, 230)


@pytest.mark.parametrize("i", wc.TIGHT)
def test_first_fit_reaches_the_last_wave_of_the_cap(kao, i):
    """Plans where some order's first fit uses exactly wave_cap waves: a cap one too small would return an error."""
    _same(wc.cap_family()[i])


@pytest.mark.parametrize("n_mv", [31, 32, 33, 64, 65])
def test_star_across_the_batch_edge(kao, n_mv):
    """One source, n_mv destinations, one placement per round: the last one falls in round n_mv - 1, on either side of the
    host's check after 32 and 64 rounds, and in wave n_mv - 1 = wave_cap - 1.  Count-only, sized by count (k = 1, no byte
    cap) and sized by bytes (k = 0, C = one partition's traffic at the source)."""
    for case in (wc.star(n_mv), wc.star(n_mv, wc.GIB, 0, 1), wc.star(n_mv, wc.GIB, wc.GIB, 0)):
        assert wc.case_cap(case) == n_mv
        wave, nw, lb = _same(case)
        assert nw == lb == n_mv
        assert sorted(wave.tolist()) == list(range(n_mv))


@pytest.mark.parametrize("name", wc.MID_CASES)
def test_mid_plan_bit_for_bit(kao, name):
    """1,000 moving partitions on 40 brokers (four workgroups; the largest degree is 95, so at least three batches of 32 rounds): log-uniform sizes, all equal, equal
    traffic codes over different sizes, oversized partitions, a tenth empty; byte cap alone, both caps, count cap alone; and the
    count-only planner at k = 1 on the same rows."""
    case = wc.mid_case(name)
    assert wc.n_moving(case) == 1000
    _same(case)


@pytest.mark.parametrize("name", wc.SHAPE_NAMES)
def test_row_shapes_bit_for_bit(kao, name):
    """Width 8 with nine participants, RF 2 padded to width 8, current[p][0] == NONE with followers, RF changes both ways,
    255 / 256 / 257 moving partitions among a partition count that is no multiple of 64, and seeds 0, 2^63, 2^64 - 1."""
    case = next(c for c in wc.shape_cases() if c[0] == name)
    _same(case)

