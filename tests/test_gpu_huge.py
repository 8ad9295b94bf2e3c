"""GPU tests at the top of the size range: topics of more than 2^20 replica slots (up to the 4,000,000 that kao_model.cpp::validate
accepts), where per-rack counts pass 65,535, partition indices pass 2^16 .. 2^20 and K-bound's subgradients grow with n = P * RF.
Every result is checked against the project's own references through the C ABI: the C port (oracle/kao_port.c: K-eval, K-search /
K-init replay, K-bound replay, exact dual value) and the oracle's Lagrangian dual (oracle/kao_lp.py::exact_dual_value).  Topics are
built by tests/huge_ref.py (numpy, well under a second at 10^6 slots).  The scalar references are single-threaded C that releases
the GIL, so the slow ones run on a thread pool beside the device work."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import random_candidates
from huge_ref import NONE, check_validate_limits, huge_topic

pytestmark = pytest.mark.gpu

TWO20, TWO21 = 1 << 20, 1 << 21


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(max_workers=8) as ex:
        yield ex


def _feasible_topic(kao, *args, **kw):
    ot, pt = huge_topic(*args, **kw)
    check_validate_limits(ot)
    assert kao.check_infeasible(pt) == "", kao.check_infeasible(pt)
    return ot, pt


# ------------------------------------------------------------------------------- K-eval (kao_evaluate_batch)
@pytest.mark.parametrize("B,R,P,rf,new_rf", [
    (400, 2, 350_000, 3, None),      # n = 1,050,000 > 2^20; 525,000 replicas per rack
    (200, 4, 700_000, 3, None),      # n = 2,100,000 ~ 2^21
    (300, 3, 350_000, 6, None),      # n = 2,100,000, the 8-slot instantiation (RF 6)
    (160, 4, 500_000, 8, None),      # n = 4,000,000: validate's limit, RF 8, 25,000 per broker
    (240, 2, 500_000, 4, 3),         # RF 4 -> 3, n = 1,500,000 on 2 racks
])
def test_eval_above_2_20_slots_matches_the_port(kao, kp, B, R, P, rf, new_rf):
    """K-eval bit-exact against the C evaluator (objective and all eight violation counts) on random candidates -- mutations, empty
    slots, out-of-range ids, duplicates -- of topics beyond 2^20 slots.  A batch this small runs on the cooperative path (one workgroup
    per candidate); per-rack totals exceed 65,535 on every shape."""
    ot, pt = huge_topic(B, R, P, rf, removed=[1, B // 2 + 1], added=[(B, 1 % R)], new_rf=new_rf, drift=0.1, seed=B)
    check_validate_limits(ot)
    n = P * ot.rf
    assert n > TWO20 and n // R > 65535
    t0 = time.perf_counter()
    cands = random_candidates(ot, 3, seed=n % 1000, p_mut=0.1, p_none=0.01)
    obj, viol = kao.evaluate_batch(pt, cands)
    t1 = time.perf_counter()
    for i in range(len(cands)):
        o, v = kp.port_eval(ot, cands[i])
        assert (int(obj[i]), viol[i].tolist()) == (o, v.tolist()), (i, B, R, P, rf)
    print(f"K-eval {B} x {P} x RF {ot.rf} (n {n}): GPU {t1 - t0:.2f} s, port {time.perf_counter() - t1:.2f} s")


def test_eval_one_wavefront_path_per_rack_above_65535(kao, kp):
    """More candidates than 4 per compute unit: every wavefront evaluates its own candidates (no cooperation), with the unpacked
    wavefront sums and the overflow check of P * RF > 65,535.  2 racks of 105,000 replicas each; each output is compared with the C
    evaluator's value of its candidate (eight distinct candidates, tiled)."""
    ot, pt = huge_topic(100, 2, 70_000, 3, removed=[7], added=[(100, 1)], drift=0.2, seed=5)
    check_validate_limits(ot)
    base = random_candidates(ot, 8, seed=11, p_mut=0.2, p_none=0.02)
    n_cand = 1100                                       # > 4 x 256 compute units: kao_eval_plan_run leaves the cooperative path
    cands = np.ascontiguousarray(np.tile(base, (n_cand // 8 + 1, 1, 1))[:n_cand])
    obj, viol = kao.evaluate_batch(pt, cands)
    ref = [kp.port_eval(ot, base[j]) for j in range(8)]
    for i in range(n_cand):
        o, v = ref[i % 8]
        assert (int(obj[i]), viol[i].tolist()) == (o, v.tolist()), i


def test_eval_per_broker_counter_boundary(kao, kp):
    """The per-broker counters are 16-bit halves (replicas | leaders << 16): exactly 65,535 replicas -- and 65,535 leaders -- on one
    broker are evaluated exactly; 65,536 are refused with KAO_ERR_UNSUPPORTED instead of carrying into the other half."""
    B, P = 8, 70_000
    ot, pt = huge_topic(B, 2, P, 2)
    p = np.arange(P)
    other = (1 + p % 7).astype(np.uint16)
    other2 = (1 + (p + 1) % 7).astype(np.uint16)

    def follower_on_0(k):     # broker 0 follows in the first k partitions, never leads
        c = np.stack([other, other2], axis=1)
        c[:k, 1] = 0
        return c

    def leader_on_0(k):       # broker 0 leads the first k partitions (and holds no other replica)
        c = np.stack([other, other2], axis=1)
        c[:k, 0] = 0
        c[:k, 1] = other[:k]
        return c

    ok = np.stack([follower_on_0(65535), leader_on_0(65535)]).reshape(2, -1)
    obj, viol = kao.evaluate_batch(pt, ok)
    for i in range(2):
        o, v = kp.port_eval(ot, ok[i])
        assert (int(obj[i]), viol[i].tolist()) == (o, v.tolist()), i
    for make in (follower_on_0, leader_on_0):
        with pytest.raises(kao.KaoError) as e:
            kao.evaluate(pt, make(65536))
        assert e.value.code == -2, make.__name__
        with pytest.raises(kao.KaoError) as e:   # one bad candidate in a batch fails the batch
            kao.evaluate_batch(pt, np.stack([ok[0], make(65536).reshape(-1)]))
        assert e.value.code == -2, make.__name__


# ------------------------------------------------------------------------------- K-search / K-init on the global-memory path (Session)
def _decommission(kao):
    """1000 brokers / 20 racks x 360,000 partitions RF 3 (1,080,000 slots), 31 brokers replaced (33,480 holes)."""
    gone = list(range(5, 1000, 33))
    return _feasible_topic(kao, 1000, 20, 360_000, 3, removed=gone, added=[(1000 + i, b % 20) for i, b in enumerate(gone)])


def test_k_search_and_k_init_above_2_20_slots(kao, kp, monkeypatch, pool):
    """A decommission topic beyond 2^20 slots with more than 65,535 partitions and tens of thousands of holes: two launches of
    K-init + K-search, bit for bit the scalar replay (final state, best snapshot, V, objective, applied moves) for two restarts; the
    multi-wavefront K-init fill (default KAO_INIT_WAVES) and the one-wavefront fill (KAO_INIT_WAVES=0) give identical restarts; and
    a priced team run (set_prices, team 4) against PortRun."""
    ot, pt = _decommission(kao)
    assert pt.n_partitions > 65535 and int((ot.current == NONE).sum()) > 30000
    seed, iters = 9091, 24
    tseed = seed ^ 0x9E3779B97F4A7C15
    t0 = time.perf_counter()
    refs = {rho: pool.submit(kp.port_search, ot, tseed, rho, 2, iters) for rho in (0, 2)}
    rng = np.random.default_rng(8)
    prices = ((rng.integers(-8, 9, ot.n_brokers) * 16384).astype(np.int32), (rng.integers(-4, 5, ot.n_brokers) * 16384).astype(np.int32),
              (rng.integers(-2, 3, ot.n_racks) * 16384).astype(np.int32))

    def priced_ref():
        run = kp.PortRun(ot, tseed, 1, team=4)
        run.launch(0, iters, prices=prices); run.launch(1, iters, prices=prices)
        out = run.read()
        run.close()
        return out
    pref = pool.submit(priced_ref)
    sigs = {}
    for waves in (None, "0"):
        if waves is None: monkeypatch.delenv("KAO_INIT_WAVES", raising=False)
        else: monkeypatch.setenv("KAO_INIT_WAVES", waves)
        with kao.Session([pt], seed=seed, restarts=3, iters_per_launch=iters, team=1) as s:
            assert s.stats()["lds_bytes_search"] < 48 * 1024             # the global-memory path
            s.step(2)
            assert s.stats()["drift"] == 0
            st = [s.restart_state(0, rho) for rho in range(3)]
        sigs[waves] = [(d["final"].tobytes(), d["best"].tobytes(), d["best_obj"], d["V"], d["obj"], d["n_accept"]) for d in st]
    monkeypatch.delenv("KAO_INIT_WAVES", raising=False)
    assert sigs[None] == sigs["0"], [rho for rho in range(3) if sigs[None][rho] != sigs["0"][rho]]
    with kao.Session([pt], seed=seed, restarts=3, iters_per_launch=iters, team=4) as s:
        s.set_prices(0, *prices)
        s.step(2)
        assert s.stats()["drift"] == 0
        dp = s.restart_state(0, 1)
    t1 = time.perf_counter()
    for rho, f in refs.items():
        ref, dev = f.result(), st[rho]
        assert np.array_equal(dev["final"], ref["final"]) and np.array_equal(dev["best"], ref["best"]), rho
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), rho
        obj, viol = kp.port_eval(ot, dev["final"])
        assert (obj, int(viol[0])) == (dev["obj"], dev["V"]), rho
    ref = pref.result()
    assert np.array_equal(dp["final"], ref["final"]) and np.array_equal(dp["best"], ref["best"])
    assert (dp["best_obj"], dp["V"], dp["obj"], dp["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"])
    print(f"K-search 1000 x 360,000: GPU + replays {t1 - t0:.2f} s, rest {time.perf_counter() - t1:.2f} s")


# ------------------------------------------------------------------------------- K-bound (kao_dual_bound) above 2^20 slots
def _bound_chunk(monkeypatch, chunk):
    """As test_gpu_parity.py: None = the library's choice, "0" = k_bound's single workgroup, "64" = k_bound_multi in slices of 64,
    "step" / "step64" = k_bound_step (one launch per iteration)."""
    monkeypatch.delenv("KAO_BOUND_CHUNK", raising=False)
    monkeypatch.delenv("KAO_BOUND_MULTI", raising=False)
    if chunk is None:
        return
    if chunk.startswith("step"):
        monkeypatch.setenv("KAO_BOUND_MULTI", "0")
        chunk = chunk[4:]
    if chunk:
        monkeypatch.setenv("KAO_BOUND_CHUNK", chunk)


def _port_replay(kp, ot, target, iters, launches):
    st = kp.DualState(ot)
    for _ in range(launches):
        st = kp.port_dual_bound(ot, target, iters, st)
        if st.flags & 7:
            break
    return st


def test_dual_bound_replay_above_2_20_slots(kao, kp, monkeypatch, pool):
    """K-bound against its scalar replay beyond 2^20 slots, with few brokers (band ends 10,500 .. 25,000) on 2 to 4 racks, one RF
    4 -> 3 change: identical iteration count, flags, best dual value and multipliers after 2 launches of 12 iterations.  The target
    is 3 below the floor of the LP value, which no dual value reaches: every iteration runs, so the direction memory, the level
    control and the rounding probes all take part.  The first shape runs under every driver."""
    shapes = [  # (B, R, P, rf, new_rf)
        (100, 2, 350_000, 3, None),     # n = 1,050,000, rep band 10,500
        (60, 3, 500_000, 3, None),      # n = 1,500,000, 25,000
        (84, 4, 699_050, 3, None),      # n = 2,097,150 = 2^21 - 2, 24,966
        (80, 4, 350_000, 4, 3),         # n = 1,050,000 after RF 4 -> 3
    ]
    iters, launches = 12, 2
    cases = []
    for B, R, P, rf, new_rf in shapes:
        ot, pt = _feasible_topic(kao, B, R, P, rf, new_rf=new_rf, drift=0.2, seed=P)
        assert TWO20 < P * ot.rf < TWO21
        _bound_chunk(monkeypatch, None)
        target = int(np.floor(kao.lp_bound(pt)["dual"])) - 3
        cases.append((ot, pt, target, pool.submit(_port_replay, kp, ot, target, iters, launches)))
    t0 = time.perf_counter()
    for i, (ot, pt, target, fut) in enumerate(cases):
        for chunk in ([None, "0", "64", "step", "step64"] if i == 0 else [None]):
            _bound_chunk(monkeypatch, chunk)
            got = kao.dual_bound(pt, target, iters=iters, launches=launches)
            st = fut.result()
            tag = (i, chunk, ot.n_brokers, ot.n_partitions, ot.rf)
            assert st.iters == iters * launches and not st.flags & 7, tag       # the target is out of reach: no early stop
            assert (got["iters"], got["flags"], got["best_dual"]) == (st.iters, st.flags, st.best_L), (tag, got["iters"], got["flags"], got["best_dual"], st.best_L)
            assert got["a"].tolist() == st.a.tolist() and got["l"].tolist() == st.l.tolist(), tag
            assert got["g"].tolist() == st.g[:ot.n_racks].tolist(), tag
            assert got["bound"] == st.bound > target, tag
    print(f"K-bound replays: {time.perf_counter() - t0:.2f} s after the LP targets")


def test_dual_bound_limits_at_2_21_slots(kao, ko):
    """dual_supported: a topic of exactly 2^21 slots is inside K-bound, one partition more is not -- kao_dual_bound refuses it and a
    session skips it with flag 8.  8,000 brokers on 2^21 slots are inside the proven headroom (|s|_1 from the band ends, not from
    65,535 per entry) and accepted."""
    ot, pt = huge_topic(80, 4, TWO21 // 4, 4)
    check_validate_limits(ot)
    got = kao.dual_bound(pt, kao.upper_bound(pt), iters=1)
    assert got["iters"] == 1 and not got["flags"] & 4
    over_o, over = huge_topic(80, 4, TWO21 // 4 + 1, 4)
    check_validate_limits(over_o)
    with pytest.raises(kao.KaoError) as e:
        kao.dual_bound(over, kao.upper_bound(over), iters=1)
    assert e.value.code == -2
    from conftest import to_product_topic
    kat = to_product_topic(ko.readme_example())
    with kao.Session([over, kat], restarts=8, iters_per_launch=8) as s:
        s.step(1)
        s.bound_step([kao.upper_bound(over), 58], 100)
        b = s.bounds()
        assert b["flags"][0] == 8 and b["iters"][0] == 0 and b["upper_bound"][1] == 58
    wide_o, wide = huge_topic(8000, 20, TWO21 // 4, 4)
    check_validate_limits(wide_o)
    got = kao.dual_bound(wide, kao.upper_bound(wide), iters=1)
    assert got["iters"] == 1 and not got["flags"] & 4


# ------------------------------------------------------------------------------- KAO-LP certificate (kao_lp_bound) above 2^20 slots
@pytest.mark.parametrize("B,R,P", [(400, 8, 350_000), (64, 4, 400_000)])
def test_lp_certificate_is_the_exact_dual_value(kao, kp, B, R, P, pool):
    """kao_lp_bound solves the LP, takes its row duals as multipliers (returned as they came from the LP, before K-bound's common
    shifts) and runs ONE K-bound iteration from them: the dual value at the shifted point, then the two rounding probes at the
    quarter / half grid of the stepped point; best_dual is the least of the three.  oracle/kao_lp.py::exact_dual_value runs the same
    iteration in the C port from the same multipliers, in the same integers, so the device value must EQUAL it: a value below it would
    be a certificate no Lagrangian function gives (a false proof), one above it a lost bound.  The bound is floor(best_dual / 65536)
    and is never below a verified incumbent."""
    import kao_lp as kl
    ot, pt = _feasible_topic(kao, B, R, P, 3, drift=0.2, seed=B + P)
    assert P * 3 > TWO20
    t0 = time.perf_counter()
    lp = kao.lp_bound(pt)
    mult = np.concatenate([lp["a"], lp["l"], lp["g"]])
    assert np.abs(mult).max() <= 1 << 26          # inside K-bound's clamp: the device starts from exactly these multipliers
    exact = pool.submit(kl.exact_dual_value, ot, lp["a"], lp["l"], lp["g"])
    inc = kao.lp_round(pt)                         # an incumbent: the perturbed LP's iterate, rounded (kao_lp_round)
    t1 = time.perf_counter()
    obj, viol = kp.port_eval(ot, inc["assignment"])
    assert viol[0] == 0 and obj == inc["objective"]
    ev = exact.result()
    assert lp["best_dual"] == ev * 65536, (lp["best_dual"], ev * 65536)
    assert lp["bound"] == lp["best_dual"] // 65536 >= obj, (lp["bound"], obj)
    print(f"LP certificate {B} x {P}: bound {lp['bound']} (LP {lp['dual']:.3f}), incumbent {obj}; GPU {t1 - t0:.2f} s, "
          f"port {time.perf_counter() - t1:.2f} s more")


# ------------------------------------------------------------------------------- kao_solve on a huge topic under a short deadline
def test_huge_topic_under_a_limit_below_the_lp_estimate(kao, kp):
    """1000 brokers / 20 racks x 499,990 partitions RF 3 (1,499,970 slots), drifted, with a time limit (1.0 s) below the schedule's
    estimate of one LP solve (about 1.1 s: kao_solve.cpp lp_est_s).  The LP cannot run alone from the start, and it would only start
    once KAO-CX has run the incumbent to a fixpoint; K-search is paused from the first feasible incumbent on.  KAO-CX must therefore
    run (before the fix it waited for that LP, and the solve sat idle until the deadline).  The plan is feasible under the C
    evaluator, no worse than its bound, and better than that of a one-launch solve of the same topic and seed."""
    ot, pt = _feasible_topic(kao, 1000, 20, 499_990, 3, drift=0.01, seed=17)
    r1 = kao.solve([pt], seed=4, max_launches=1)[0]        # (also the warm allocation of the big arenas)
    r = kao.solve([pt], seed=4, time_limit_s=1.0)[0]
    tm, lp = kao.last_solve_timing(), kao.last_solve_lp()
    print(f"1000 x 499,990 under 1 s: {r.status} {r.objective} <= {r.upper_bound} (best at {r.seconds_to_best:.2f} s); one launch: {r1.status} "
          f"{r1.objective}; launches {tm['launches']} CX calls {tm['cx_calls']} gains {tm['cx_gains']} LP solves {lp['solves']} iterations {lp['iterations']}")
    for res in (r1, r):
        if res.status != "NO_FEASIBLE":
            obj, viol = kp.port_eval(ot, res.assignment)
            assert viol[0] == 0 and obj == res.objective <= res.upper_bound <= kao.upper_bound(pt), res.status
    assert r.status != "NO_FEASIBLE"
    # progress after the first feasible incumbent, by counts: KAO-CX ran and improved the incumbent
    assert tm["cx_calls"] > 0 and tm["cx_gains"] > 0, tm
    assert r1.status == "NO_FEASIBLE" or r.objective > r1.objective, (r.objective, r1.objective)
