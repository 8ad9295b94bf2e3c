"""KAO-LP on every kernel path it dispatches: the device trace (kao_lp.hip + kao_chol.hip) against the scalar restatement
(oracle/kao_lp_port.c) iterate by iterate, at shapes picked so that each instantiation lp_factor / lp_open choose is reached -- the
rack-block tile counts, the broker kernel's column forms at their boundaries, one to four wavefronts per broker workgroup, the
LDS-tiled rack kernel beyond 64 racks, Cholesky tile counts of production size -- and the dense kernels alone at production orders.
An LP kernel that is slightly wrong costs iterations, not answers (the certificate is K-bound's exact dual value, the rounded plan is
scored exactly), so only a comparison like this one notices it.  lp_paths() restates the dispatch rules; the CPU test below checks
that the shapes here reach every one of them."""
import math

import numpy as np
import pytest

from conftest import have_gpu, to_product_topic
from lp_helpers import drift_topic, otopic, trace_close

gpu = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not have_gpu(), reason="needs a GPU")

LDS_PAIR_BYTES = 150 * 1024      # kao_lp.hip lp_open: one broker's row pair (2 mc doubles) per wavefront must fit this


def lp_paths(B, R, NJ, waves=None):
    """What KAO-LP launches for a topic of B brokers, R racks and current RF NJ (mc = 3R + 2B coupling rows), restating
    kafka_assignment_optimizer_amd/csrc/kao_lp.hip:
      broker form   lp_factor (about line 1384) and k_lp_schur_broker (about line 444): nc = 2 NJ + 2 R coupling columns per
                    partition; "<4>" for nc <= 64, "<4,2>" up to 128, "walk" (the one-column walk inside <4,2>) beyond;
      rack form     lp_factor (about lines 1386-1400): T16 = ceil(2R / 16) tiles of 16 on k_lp_schur_rack_mfma<T16> for T16 <= 8,
                    dealt to rack_mfma_shares(T16) = 1 / 2 / 3 / 4 shares of tile rows (about line 700); beyond, k_lp_schur_rack with
                    rack_tile = clamp(65536 // (8 (6 * 2R + R)), 1, 16) partitions in LDS (lp_open, about line 1557);
      broker_waves  lp_open (about line 1555): clamp(150 KiB // (2 mc * 8), 1, 4), lowered by KAO_LP_BROKER_WAVES (`waves`);
      tiles         mcp / 64, mcp = mc rounded up to 64: k_chol_first, tiles - 1 launches of k_chol_step, k_trsv's workgroups.
    Returns (broker form, rack form, T16 or rack_tile, shares, broker_waves, tiles)."""
    mc = 3 * R + 2 * B
    nc = 2 * NJ + 2 * R
    broker = "<4>" if nc <= 64 else "<4,2>" if nc <= 128 else "walk"
    t16 = (2 * R + 15) // 16
    if t16 <= 8:
        rack, size, shares = "mfma", t16, 1 if t16 <= 4 else 2 if t16 <= 6 else 3 if t16 == 7 else 4
    else:
        rack, size, shares = "tiled", max(1, min(16, 65536 // (8 * (6 * 2 * R + R)))), 0
    bw = max(1, min(4, LDS_PAIR_BYTES // (2 * mc * 8)))
    if waves is not None:
        bw = max(1, min(bw, waves))
    return broker, rack, size, shares, bw, (mc + 63) // 64


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
# (id, B, R, P, rf, new_rf, KAO_LP_BROKER_WAVES, max_iters (0: to convergence), broker weights).  B >= R (synthetic.make_cluster).
TRACE = [
    ("t16_2", 120, 12, 1000, 3, None, None, 0, False),
    ("t16_3_north_star_racks", 100, 20, 1000, 3, None, None, 0, False),
    ("t16_6_waves3", 176, 44, 900, 3, None, 3, 0, False),
    ("cols64", 116, 29, 1000, 3, None, None, 0, False),
    ("cols128_waves2", 122, 61, 900, 3, None, 2, 0, False),
    ("cols130", 124, 62, 900, 3, None, None, 0, False),
    ("tiled65", 130, 65, 1000, 3, None, None, 0, False),
    ("tiled100_waves1", 200, 100, 1000, 3, None, 1, 0, False),
    ("tiled255", 510, 255, 600, 3, None, None, 3, False),
    ("r1", 100, 1, 1000, 3, None, None, 0, False),
    ("r2", 100, 2, 1000, 3, None, None, 0, False),
    ("rf1", 100, 5, 1000, 1, None, None, 0, False),
    ("rf2_t16_7", 150, 50, 800, 2, None, None, 0, False),
    ("rf5_t16_5", 120, 40, 800, 5, None, None, 0, False),
    ("rf8", 100, 10, 600, 8, None, None, 0, False),
    ("rf2to3", 120, 6, 1000, 2, 3, None, 0, False),
    ("rf4to3", 120, 6, 1000, 4, 3, None, 0, False),
    ("nj8_cols64", 96, 24, 600, 8, None, None, 0, False),
    ("weights", 120, 12, 800, 3, None, None, 0, True),
]
PERTURBED = [("pert_r20", 100, 20, 1000), ("pert_r100", 200, 100, 1000)]
PERT_SENS = 100         # test_perturbed_lp_trace: device vs restatement within this many times the restatement's own last-digit sensitivity
# production sizes, two iterations: the north star itself (33 tiles, 4 wavefronts) and 1,250 brokers (40 tiles, 3 wavefronts)
PRODUCTION = [("north_star", 1000, 20, 100_000), ("b1250", 1250, 10, 50_000)]
DENSE_N = [2112, 4864, 9600]     # 33, 76 and 150 tiles (9,600 = the LP's LDS ceiling: about 4,700 brokers)


def test_the_shapes_reach_every_dispatch_path():
    """CPU: the parametrisation of this module covers every rack-block tile count 1..8 and share count, the tiled rack kernel at
    rack_tile 9 / 6 / 2, the broker kernel's 64- / 128-column boundaries and the walk just beyond, one to four wavefronts per broker
    workgroup, and Cholesky tile counts of 33+ (LP) and 76+ / 150 (dense kernels)."""
    paths = [lp_paths(B, R, rf, w) for (_, B, R, P, rf, nrf, w, _, _) in TRACE]
    paths += [lp_paths(B, R, 3) for (_, B, R, P) in PERTURBED + PRODUCTION]
    mfma = {p[2] for p in paths if p[1] == "mfma"}
    assert mfma == set(range(1, 9)), sorted(mfma)
    assert {p[3] for p in paths if p[1] == "mfma"} == {1, 2, 3, 4}
    assert {9, 6, 2} <= {p[2] for p in paths if p[1] == "tiled"}
    cols = {2 * rf + 2 * R for (_, B, R, P, rf, nrf, w, _, _) in TRACE}
    assert {64, 128, 130} <= cols
    assert {p[0] for p in paths} == {"<4>", "<4,2>", "walk"}
    assert {p[4] for p in paths} == {1, 2, 3, 4}
    assert max(p[5] for p in paths) >= 33
    assert [n // 64 for n in DENSE_N] == [33, 76, 150]
    assert lp_paths(4700, 20, 3)[4] == 1 and 2 * (3 * 20 + 2 * 4700) * 8 <= LDS_PAIR_BYTES     # the LP's ceiling is the dense sizes' top
    # the rules themselves at a few known points (DESIGN / the issue's table)
    assert lp_paths(1000, 20, 3) == ("<4>", "mfma", 3, 1, 4, 33)
    assert lp_paths(1250, 10, 3)[4:] == (3, 40) and lp_paths(1650, 10, 3)[4:] == (2, 53) and lp_paths(2400, 10, 3)[4:] == (1, 76)
    assert lp_paths(130, 65, 3)[1:3] == ("tiled", 9) and lp_paths(200, 100, 3)[1:3] == ("tiled", 6) and lp_paths(510, 255, 3)[1:3] == ("tiled", 2)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    return k


def _topic(ko, B, R, P, rf, new_rf=None):
    return drift_topic(ko, B, R, P, rf=rf, new_rf=new_rf)


def _multipliers_close(d, r):
    for k in ("a", "l", "g"):   # fixed point, 2^-16; the optimal duals are a face: the last iterates drift along it (test_gpu_lp.py)
        assert np.abs(d[k].astype(np.int64) - r[k]).max() <= 8192, k


def _certificate_is_the_exact_dual_value(kao, kp, pt, ot, max_iters=0):
    """K-bound's dual value at the multipliers kao_lp_bound hands over equals the scalar restatement's evaluation there, bit for bit."""
    b = kao.lp_bound(pt, max_iters=max_iters)
    st = kp.DualState(ot)
    st.a[:] = b["a"]; st.l[:] = b["l"]; st.g[:len(b["g"])] = b["g"]
    kp.port_dual_bound(ot, 0, 1, st)
    assert st.best_L == b["best_dual"], (st.best_L, b["best_dual"])
    return b


@gpu
@needs_gpu
@pytest.mark.parametrize("case", TRACE, ids=[c[0] for c in TRACE])
def test_lp_trace_on_every_path(kao, ko, kp, monkeypatch, case):
    """Device trace == restatement to 1e-7 per iterate, final multipliers within test_gpu_lp.py's margin, the certificate's dual value
    bit-exact at the device's multipliers; up to 64 racks the LP value is also HiGHS's (beyond, HiGHS takes minutes: the restatement's
    converged value is the reference)."""
    import kao_lp as kl
    name, B, R, P, rf, new_rf, waves, maxit, weighted = case
    if waves is not None:
        monkeypatch.setenv("KAO_LP_BROKER_WAVES", str(waves))
    pt, ot = _topic(ko, B, R, P, rf, new_rf)
    if weighted:
        rng = np.random.default_rng(11)
        ot.broker_w = rng.integers(0, 6, ot.n_brokers).astype(np.int32)
        ot.broker_wl = rng.integers(0, 4, ot.n_brokers).astype(np.int32)
        pt = to_product_topic(ot)
    assert ot.rf_cur == rf      # NJ: a changed RF keeps the current assignment's columns
    d = kao.lp_trace(pt, max_iters=maxit or 80)
    r = kl.port_solve(ot, maxit=maxit or 80)
    print(f"{name}: paths {lp_paths(B, R, ot.rf_cur, waves)} device {d['iterations']} iterations status {d['status']}, restatement "
          f"{r['iterations']} status {r['status']}, LP {r['dual']:.6f}")
    trace_close(d["trace"], r["trace"])
    if maxit:    # iteration-limited: the same iterate, nowhere near the optimum
        assert d["iterations"] == r["iterations"] == maxit
        _certificate_is_the_exact_dual_value(kao, kp, pt, ot, max_iters=maxit)
        return
    assert d["status"] == 0 and r["status"] == 0
    _multipliers_close(d, r)
    assert abs(d["dual"] - r["dual"]) <= 1e-6 * max(1.0, abs(r["dual"])), (d["dual"], r["dual"])
    b = _certificate_is_the_exact_dual_value(kao, kp, pt, ot)
    if R <= 64:
        val, _, _, _ = kl.solve_highs(kl.build(ot))
        assert abs(d["dual"] - val) < 1e-3, (d["dual"], val)
        assert b["bound"] == math.floor(val + 1e-6), (b["bound"], val)


def _rel(a, b):
    """relative difference of two trace rows in mu, primal and dual objective (trace_close's measures)"""
    return max(abs(a[0] - b[0]) / b[0], abs(a[1] - b[1]) / max(1.0, abs(b[1])), abs(a[2] - b[2]) / max(1.0, abs(b[2])))


@gpu
@needs_gpu
@pytest.mark.parametrize("case", PERTURBED, ids=[c[0] for c in PERTURBED])
def test_perturbed_lp_trace(kao, ko, kp, monkeypatch, case):
    """The perturbed LP production rounds (KAO_LP_TRACE_PERT=-1: kao_solve's own eps = min(1e-4, 1.5 / slots), salt 0) to convergence,
    on 20 racks (the north star's rack block) and on 100 (the LDS-tiled rack kernel).

    Device and restatement agree to 1e-12 .. 1e-10 per iterate until the first SHORT BLOCKED STEP near the vertex (restatement's step
    trace: on 20 racks iteration 7 goes 0.09 / 0.03 of the way, blocked by a variable at 1.8e-7; on 100 racks iteration 8, 0.16 / 0.12,
    blocked by one at 1.9e-8).  The length of such a step is x_i / |dx_i| of a variable that close to its bound, and dx_i is where the
    ill-conditioned normal equations lose their digits: the next iterates part by 1e-7 (20 racks) and 1e-3 (100 racks).  The
    restatement parts from ITSELF in the same place when every cost perturbation changes in its last digits (eps x (1 + 1e-14) or
    (1 + 1e-13)).  So every iterate down to mu = 1e-6 (trace_close's floor) is held to 1e-7, or to PERT_SENS times the restatement's
    own divergence under those changes so far where that is larger; the ends must agree in status, iteration count and dual value."""
    import kao_lp as kl
    name, B, R, P = case
    monkeypatch.setenv("KAO_LP_TRACE_PERT", "-1")
    pt, ot = _topic(ko, B, R, P, 3)
    eps = min(1e-4, 1.5 / (P * ot.rf))
    d = kao.lp_trace(pt, tol=1e-8, max_iters=150)
    r = kl.port_solve(ot, tol=1e-8, maxit=150, pert=eps, salt=0)
    selfs = [kl.port_solve(ot, tol=1e-8, maxit=150, pert=eps * (1 + q), salt=0)["trace"] for q in (1e-14, 1e-13)]
    print(f"{name}: device {d['iterations']} iterations status {d['status']}, restatement {r['iterations']} status {r['status']}")
    assert abs(len(d["trace"]) - len(r["trace"])) <= 1
    sens = 0.0
    for i, (a, b) in enumerate(zip(d["trace"], r["trace"])):
        if b[0] < 1e-6:
            break
        sens = max([sens] + [_rel(t[i], b) for t in selfs if i < len(t)])
        print(f"  it {i:3d} mu {b[0]:.3e} device {_rel(a, b):.2e} restatement under a last-digit change {sens:.2e}")
        trace_close(a[None], b[None], rel=max(1e-7, PERT_SENS * sens))
        if i < 7:
            assert _rel(a, b) <= 1e-7
    assert d["status"] == 0 and r["status"] == 0 and abs(d["iterations"] - r["iterations"]) <= 1
    assert abs(d["dual"] - r["dual"]) <= 1e-6 * max(1.0, abs(r["dual"])), (d["dual"], r["dual"])


@gpu
@needs_gpu
@pytest.mark.parametrize("case", PRODUCTION, ids=[c[0] for c in PRODUCTION])
def test_lp_trace_at_production_size(kao, ko, kp, case):
    """Two iterations at production size (the restatement's dense Cholesky is O(mc^3) on one core): the north star (1000 x 100,000,
    20 racks: T16 = 3, 4 wavefronts, 33 Cholesky tiles) and 1,250 brokers (3 wavefronts, 40 tiles)."""
    import kao_lp as kl
    from kafka_assignment_optimizer_amd import synthetic as sy
    name, B, R, P = case
    if name == "north_star":
        pt = sy.north_star_topic("drift100k")
        ot = otopic(ko, pt)
    else:
        pt, ot = _topic(ko, B, R, P, 3)
    assert (pt.n_brokers, pt.n_racks, pt.n_partitions) == (B, R, P)
    d = kao.lp_trace(pt, max_iters=2)
    r = kl.port_solve(ot, maxit=2)
    print(f"{name}: paths {lp_paths(B, R, 3)}, device {d['trace'][:, :3].tolist()}")
    assert d["iterations"] == r["iterations"] == 2
    trace_close(d["trace"], r["trace"])
    _multipliers_close(d, r)


# ---- the dense kernels alone (kao_dense_spd_test) at the LP's tile counts ------------------------------------------------------
U = 2.0 ** -53
C_DENSE = 0.25    # measured worst: 0.03 (x, / (n u kappa)), 0.015 (backward), 0.15 (tile inverses, / (64 u)): see the test


def _spd(n, seed, k=256, delta=1.0):
    """A = D M D, M = G G^T / k + delta I (G: n x k standard normal): cheap to build at n = 9,600; M's condition is
    (lambda_max(G^T G / k) + delta) / delta, computed from the k x k Gram matrix; D = 10^U(-1.5, 1.5) scales the rows badly."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, k))
    M = (G @ G.T) / k
    M[np.diag_indices(n)] += delta
    kappa = (np.linalg.eigvalsh(G.T @ G / k).max() + delta) / delta
    dsc = 10.0 ** rng.uniform(-1.5, 1.5, n)
    A = M * dsc[:, None] * dsc[None, :]
    return A, dsc, kappa, rng


@gpu
@needs_gpu
@pytest.mark.parametrize("n", DENSE_N)
def test_dense_kernels_at_production_tile_counts(kao, n):
    """The factor, the tiles' inverses and the solution at 33, 76 and 150 tiles (one k_chol_first, n / 64 - 1 k_chol_step launches,
    k_chol_mirror, n / 64 k_trsv workgroups).  Backward errors within C_DENSE n u, on A and on the equilibrated D^-1 A D^-1; forward
    errors of the factor and of x (in the equilibrated variables) within C_DENSE n u kappa(M) against numpy; the tiles' inverses
    componentwise: |Linv_k L_k - I| <= C_DENSE 64 u |Linv_k| |L_k|.  Measured on the MI355X (n = 2,112 / 4,864 / 9,600; kappa(M) = 16 /
    29 / 51), as fractions of n u: backward 0.013 / 0.006 / 0.005 (equilibrated 0.015 / 0.011 / 0.007), residual 2e-7 .. 3e-8
    (equilibrated 9e-5 .. 3e-5); of n u kappa: factor 7e-4 .. 1e-4, x 0.029 / 0.018 / 0.008; tile inverses 0.12 .. 0.15 of 64 u.
    C_DENSE = 0.25 keeps a factor of 1.7 .. 8 over the worst of them."""
    A, dsc, kappa, rng = _spd(n, 200 + n // 64)
    b = rng.standard_normal(n)
    d = kao.dense_spd_test(A, b)
    L = np.tril(d.pop("factor"))      # (n x n arrays are 0.74 GB at n = 9,600: at most four are alive at once)
    x = d["x"]
    tol = C_DENSE * n * U
    R = L @ L.T
    R -= A
    e_bwd = np.abs(R).max() / np.abs(A).max()
    R /= dsc[:, None]; R /= dsc[None, :]
    Meq = A / dsc[:, None]; Meq /= dsc[None, :]
    e_bwd_eq = np.abs(R).max() / np.abs(Meq).max()
    del R
    res = A @ x - b
    e_res = np.abs(res).max() / (np.abs(A).sum(axis=1).max() * np.abs(x).max())
    e_res_eq = np.abs(res / dsc).max() / (np.abs(Meq).sum(axis=1).max() * np.abs(x * dsc).max())
    del Meq
    xn = np.linalg.solve(A, b)
    Ln = np.linalg.cholesky(A)
    Ln -= L; Ln /= dsc[:, None]
    e_fac = np.abs(Ln).max() / np.abs(L / dsc[:, None]).max()
    del Ln
    e_x = np.abs((x - xn) * dsc).max() / np.abs(xn * dsc).max()
    e_inv = 0.0
    for k in range(n // 64):
        Lk, Xk = L[k * 64:(k + 1) * 64, k * 64:(k + 1) * 64], d["linv"][k]
        assert np.abs(np.triu(Xk, 1)).max() == 0.0
        den = np.abs(Xk) @ np.abs(Lk)          # lower triangular: zero above the diagonal, where X L - I is exactly zero
        num = np.abs(Xk @ Lk - np.eye(64))
        assert num[den == 0].max(initial=0.0) == 0.0
        e_inv = max(e_inv, float((num[den > 0] / den[den > 0]).max()))
    print(f"n {n} kappa(M) {kappa:.1f}: / (n u): backward {e_bwd / (n * U):.3g} equilibrated {e_bwd_eq / (n * U):.3g} residual "
          f"{e_res / (n * U):.3g} equilibrated {e_res_eq / (n * U):.3g}; / (n u kappa): factor {e_fac / (n * U * kappa):.3g} x {e_x / (n * U * kappa):.3g}; tile inverses / (64 u) "
          f"{e_inv / (64 * U):.3g}")
    assert e_bwd <= tol and e_bwd_eq <= tol and e_res <= tol and e_res_eq <= tol, (e_bwd, e_bwd_eq, e_res, e_res_eq, tol)
    assert e_fac <= tol * kappa and e_x <= tol * kappa, (e_fac, e_x, tol * kappa)
    assert e_inv <= C_DENSE * 64 * U, e_inv


@gpu
@needs_gpu
def test_dense_kernels_pin_dependent_rows_across_tiles(kao):
    """The pinned-row rule (tests/test_gpu_lp.py test_dense_kernels_pin_a_dependent_row) at 33 tiles: rows that repeat earlier rows at
    a tile's first and last row, at the matrix's last row and twice inside one tile get L_jj = 1e64; x is finite and ~0 there, and the
    other components are numpy's solution of the system without those rows and columns."""
    n = 2112
    A, dsc, kappa, rng = _spd(n, 77)
    dup = {448: 5, 511: 200, n - 1: 1000, 1290: 1100, 1300: 1200}     # pinned row -> the earlier row it repeats
    for j, i in dup.items():
        A[j, :] = A[i, :]
        A[:, j] = A[:, i]
    b = rng.standard_normal(n)
    d = kao.dense_spd_test(A, b)
    diag = np.diag(d["factor"])
    pinned = np.flatnonzero(diag > 1e60)
    assert pinned.tolist() == sorted(dup), pinned.tolist()
    assert np.abs(diag[pinned] / 1e64 - 1.0).max() < 1e-12
    x = d["x"]
    assert np.isfinite(x).all() and np.abs(x[pinned]).max() < 1e-100
    keep = np.setdiff1d(np.arange(n), pinned)
    xr = np.linalg.solve(A[np.ix_(keep, keep)], b[keep])
    e_x = np.abs((x[keep] - xr) * dsc[keep]).max() / np.abs(xr * dsc[keep]).max()
    assert e_x <= C_DENSE * n * U * kappa, (e_x, C_DENSE * n * U * kappa)


@gpu
@needs_gpu
def test_rf_change_topics_are_certified(kao, ko, kp):
    """After an RF change (2 -> 3 here; both directions are in test_lp_trace_on_every_path) kao_solve's LP certifies the topic: 1,000
    partitions, 3,000 replica slots (above the 2,048 from which kao_solve runs the LP), OPTIMAL_PROVEN with the incumbent feasible under
    the scalar evaluator.  And a topic that is provably infeasible gets no dual certificate: on 100 brokers every broker holds exactly
    30 of the 3,000 replicas, so a 17-broker rack holds 510 where the rack band allows 500; K-bound skips such a topic (no
    iteration, best value "infinite") and
    kao_lp_bound reports no bound, where the scalar K-bound -- which never looks at feasibility -- evaluates the dual function anyway."""
    pt, ot = _topic(ko, 120, 6, 1000, 2, 3)
    assert kao.check_infeasible(pt) == ""
    r = kao.solve([pt], seed=1, stop_at_bound=1, time_limit_s=20.0)[0]
    lp = kao.last_solve_lp()
    obj, viol = kp.port_eval(ot, r.assignment)
    print(f"RF 2 -> 3: {r.status} objective {r.objective} certificate {r.upper_bound}, {int(lp['solves'])} LP solve(s)")
    assert r.status == "OPTIMAL_PROVEN" and r.objective == r.upper_bound and viol[0] == 0 and obj == r.objective, (r.status, r.objective, r.upper_bound)
    assert lp["solves"] >= 1
    bad, _ = _topic(ko, 100, 6, 1000, 2, 3)
    assert kao.check_infeasible(bad).startswith("rack 0: needs at least 510")
    b = kao.lp_bound(bad)
    assert b["bound"] == 2 ** 63 - 1 and b["best_dual"] == 0x7F7F7F7F7F7F7F7F
    assert kao.solve([bad], seed=1, stop_at_bound=1, time_limit_s=5.0)[0].status == "INFEASIBLE_PROVEN"
