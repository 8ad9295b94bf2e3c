"""KAO-CX beyond 128 nodes and on both squaring kernels, bit for bit against oracle/kao_cycle.py (tests/test_gpu_cycle.py stops at
100 brokers: row stride 64 or 128, k_cx_square_part with one pass of 16 midpoints per slice).  Here:
  b  the production split at row strides 192..320 (several passes per slice, a shorter last slice, k_cx_dist0 on two x-blocks,
     transposes of 3 x 3 .. 5 x 5 tiles, the per-partition kernels over three to five steps of 64 brokers);
  c  each squaring kernel alone, forced by the test hook KAO_CX_SQUARE_SPLIT, and the same matrices whichever ran;
  d  the largest accepted weights (255 per role, 1023 per broker);
  e  the unsplit kernel at 949 nodes against tests/golden/cx_large.npz (the oracle needs three minutes a round there);
  f  the limit, 2048 nodes: level 0 against the oracle, every squaring by single rows recomputed from the device's previous level.
Every comparison is integer equality; kao.cycle_square_plan says which kernel ran."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, to_product_topic
from test_gpu_cycle import _drifted, _same_matrices

pytestmark = pytest.mark.gpu

HOOK = "KAO_CX_SQUARE_SPLIT"
WEIGHTS = (((255, 1), (17, 16)), ((255, 0), (0, 255)))


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    return k


def _start(kp, t, launches, iters):
    r = kp.port_search(t, 3, 0, launches, iters)
    assert r["best_obj"] >= 0, "no feasible start"
    return r["best"]


def _same_rounds(kao, ko, pt, t, a, rounds, oracle):
    """kao.improve_cycles against (assignment, history) of kc.improve; feasible, the objective the verifier's."""
    Xo, hist = oracle
    Xg, obj, st = kao.improve_cycles(pt, a, rounds)
    assert np.array_equal(np.asarray(Xo).reshape(-1), Xg.reshape(-1))
    o, v = ko.verify(t, Xg)
    assert int(np.asarray(v).sum()) == 0 and o == obj == st["objective_after"]
    assert st["rounds"] == len(hist) and st["improving_rounds"] == sum("objective" in h for h in hist)
    return Xg


def _all_matrices(kao, pt, a):
    return [kao.cycle_matrices(pt, a, layer, lev) for layer in range(3) for lev in range(4)]


# ---- a. the split plan -----------------------------------------------------------------------------------------------------------
def test_square_plan(kao, monkeypatch):
    monkeypatch.delenv(HOOK, raising=False)
    assert kao.cycle_square_plan(186) == (192, 6, 32)
    assert kao.cycle_square_plan(317) == (320, 7, 48)
    for n in (897, 949, 2048):
        assert kao.cycle_square_plan(n)[:2] == ((n + 63) // 64 * 64, 1)
    monkeypatch.setenv(HOOK, "1")
    assert kao.cycle_square_plan(100)[:2] == (128, 1)
    monkeypatch.setenv(HOOK, "3")
    assert kao.cycle_square_plan(128) == (128, 3, 48)          # slices of 48, 48 and 32 midpoints


# ---- b. the production split at row strides 192 .. 320 ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape, plan", [
    ((186, 5, 400, 3), (192, 6, 32)),      # n = np: no padding
    ((187, 5, 400, 3), (256, 8, 32)),      # 63 padding rows: never a midpoint, never reachable
    ((250, 5, 500, 2), (256, 8, 32)),      # RF 2
    ((200, 5, 300, 4), (256, 8, 32)),      # RF 4
    ((200, 5, 240, 5), (256, 8, 32)),      # k_cx_edges<8>, k_cx_edges_l<8, 0>, prack_lo = prack_hi = 1
    ((200, 4, 240, 6), (256, 8, 32)),      # RF 6
    ((310, 6, 700, 3), (320, 7, 48)),      # a shorter last slice (6 x 48 + 32); k_cx_dist0 on two x-blocks
])
def test_production_split_matches_the_oracle(kao, ko, kp, monkeypatch, shape, plan):
    import kao_cycle as kc
    monkeypatch.delenv(HOOK, raising=False)
    B, R, P, rf = shape
    assert kao.cycle_square_plan(B + R + 1) == plan and plan[1] * plan[2] >= plan[0] > (plan[1] - 1) * plan[2] and plan[2] > 16
    pt, t = _drifted(ko, B, R, P, rf)
    a = _start(kp, t, 1, 512)
    rd = _same_matrices(kao, kc, pt, t, a)
    assert rd.cycle_candidates()
    rounds = 64 if B == 186 else 2             # (the oracle is pure Python)
    Xo, hist = kc.improve(t, a, rounds)
    _same_rounds(kao, ko, pt, t, a, rounds, (Xo, hist))
    if B == 186:                               # the oracle's fixpoint: no cycle candidates, so the seeds decide -- and find nothing
        assert "objective" not in hist[-1]
        fix = kc.Round(t, Xo)
        assert not fix.cycle_candidates()
        tab = kao.cycle_seeds(pt, Xo)
        assert tab.shape == (400, 38, 2) and np.array_equal(tab, fix.seed_table())     # a seed table at np >= 192


# ---- c. each squaring kernel alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, split3", [
    ((45, 5, 130, 2), (64, 2, 32)),
    ((60, 3, 200, 3), (64, 2, 32)),
    ((100, 5, 300, 3), (128, 3, 48)),          # the shorter last slice at a small size: 48, 48 and 32 midpoints
    ((186, 5, 400, 3), (192, 3, 64)),
])
def test_each_squaring_kernel_alone_matches_the_oracle(kao, ko, kp, monkeypatch, shape, split3):
    import kao_cycle as kc
    B, R, P, rf = shape
    n = B + R + 1
    pt, t = _drifted(ko, B, R, P, rf)
    a = _start(kp, t, 2, 64) if B <= 60 else _start(kp, t, 1, 512)
    rounds = 64 if B <= 60 else 2
    oracle = kc.improve(t, a, rounds)
    mats = {}
    for mode in ("1", "3", None):
        if mode is None:
            monkeypatch.delenv(HOOK)
            assert kao.cycle_square_plan(n)[1] >= 4            # production: k_cx_square_part
        else:
            monkeypatch.setenv(HOOK, mode)
            assert kao.cycle_square_plan(n) == ((split3[0], 1, split3[0]) if mode == "1" else split3)
            _same_matrices(kao, kc, pt, t, a)
            _same_rounds(kao, ko, pt, t, a, rounds, oracle)
        mats[mode] = _all_matrices(kao, pt, a)
    for mode in ("1", "3"):
        for got, want in zip(mats[mode], mats[None]):
            for x, y in zip(got, want):
                assert np.array_equal(x, y), mode


# ---- d. the largest accepted weights ---------------------------------------------------------------------------------------------
def _heavy(t, rng, i):
    t.weights = WEIGHTS[i % 2]
    t.broker_w = (rng.integers(0, 2, t.n_brokers) * 1023).astype(np.int32)
    t.broker_wl = (rng.integers(0, 2, t.n_brokers) * 1023).astype(np.int32)


def test_largest_weights_match_the_oracle(kao, ko, kp, monkeypatch):
    """Role weights of 255 and broker weights of 1023: edge costs of a few thousand, closure entries of several thousand either
    side of zero, far inside the +-2^18 of the squaring's packed key -- the oracle's int64 and the key must agree.  The start is
    searched BEFORE the weights are set: feasibility does not depend on them."""
    import kao_cycle as kc
    monkeypatch.delenv(HOOK, raising=False)
    rng = np.random.default_rng(1023)
    cases = []
    for s in range(400):
        t = ko.random_case_wide(s)
        if not 2 <= t.rf <= 4:
            continue
        r = kp.port_search(t, 3, 0, 2, 64)
        if r["best_obj"] < 0:
            continue
        cases.append((t, r["best"], 64))
        if len(cases) == 10:
            break
    assert len(cases) == 10
    _, t = _drifted(ko, 186, 5, 400, 3)
    cases.append((t, _start(kp, t, 1, 512), 2))
    n_seed_tables = lo = hi = 0
    for i, (t, a, rounds) in enumerate(cases):
        _heavy(t, rng, i)
        pt = to_product_topic(t)
        rd = _same_matrices(kao, kc, pt, t, a)
        for D in rd.DF + rd.DS + rd.DL:
            lo, hi = min(lo, int(D.min())), max(hi, int(D[D < kc.CINF // 2].max()))     # (CINF plus a negative edge is no path either)
        if not rd.cycle_candidates():
            assert np.array_equal(kao.cycle_seeds(pt, a), rd.seed_table()), i
            n_seed_tables += 1
        Xo, hist = kc.improve(t, a, rounds)
        _same_rounds(kao, ko, pt, t, a, rounds, (Xo, hist))
        if "objective" not in hist[-1]:            # the oracle's fixpoint: where no cycle is left the seeds were priced -- with these weights
            fix = _same_matrices(kao, kc, pt, t, Xo)
            if not fix.cycle_candidates():
                assert np.array_equal(kao.cycle_seeds(pt, Xo), fix.seed_table()), i
                n_seed_tables += 1
    print("closure entries", lo, "..", hi, "| seed tables", n_seed_tables)
    assert lo < -1023 and hi > 1023 and -(1 << 17) < lo and hi < (1 << 16)          # the weights were felt, and stayed inside the key
    assert n_seed_tables >= 5


# ---- e. the unsplit kernel at production size --------------------------------------------------------------------------------------
def _bands(M):
    M = np.ascontiguousarray(M)
    return np.array([np.frombuffer(hashlib.sha256(M[i:i + 64].tobytes()).digest(), dtype=np.uint8) for i in range(0, M.shape[0], 64)])


def _wrong_bands(got, want):
    return [int(b) for b in np.nonzero((_bands(got) != want).any(axis=1))[0]]


def test_unsplit_kernel_at_949_nodes_matches_the_committed_oracle_run(kao, ko, monkeypatch):
    """tests/golden/cx_large.npz (make_golden_cx_large.py, ten minutes of the oracle): one SHA-256 per 64-row band -- the
    blockIdx.y of a squaring -- of all 24 matrices, the diagonals, and two whole rounds.  The start has F cycles, so its L layer
    is built from plain replacements only; the L matrices are those of the oracle's fourth round, the first whose F closure has
    no negative diagonal entry -- the round that transposes the closure (k_cx_transpose on 15 x 15 tiles) and prices every
    variant of an L edge on it."""
    monkeypatch.delenv(HOOK, raising=False)
    g = np.load(os.path.join(GOLDEN, "cx_large.npz"))
    B, R, P, rf = (int(x) for x in g["shape"])
    n = B + R + 1
    assert (B, R, P, rf) == (940, 8, 1200, 3) and kao.cycle_square_plan(n) == (960, 1, 960)
    pt, t = _drifted(ko, B, R, P, rf)
    o, v = ko.verify(t, g["start"])
    assert int(np.asarray(v).sum()) == 0 and o == int(g["start_objective"]) == 8545
    # the round that builds L on the transposed closure: F without a negative diagonal entry at every level
    assert int(g["l_round"]) == 3 and (g["diag_l_round"][0, 1:, :B] >= 0).all() and (g["diag"][0, 1:, :B] < 0).any()
    wrong = []
    for layer in range(3):
        a = g["l_start"] if layer == 2 else g["start"]
        for lev in range(4):
            d, m, s = kao.cycle_matrices(pt, a, layer, lev)
            assert d.dtype == np.int32 and m.dtype == np.int32 and s.dtype == np.uint32 and d.shape == m.shape == s.shape == (n, n)
            ref_diag = g["diag_l_round"][2, lev] if layer == 2 else g["diag"][layer, lev]
            if not np.array_equal(np.diag(d), ref_diag):
                wrong.append(("diag", layer, lev, np.nonzero(np.diag(d) != ref_diag)[0][:8].tolist()))
            wrong += [("dist", layer, lev, b) for b in _wrong_bands(d, g["bands_dist"][layer, lev])]
            if lev:
                wrong += [("mid", layer, lev, b) for b in _wrong_bands(m, g["bands_mid"][layer, lev])]
            else:
                wrong += [("slot", layer, b) for b in _wrong_bands(s, g["bands_slot"][layer])]
    assert not wrong, wrong[:40]
    hist = json.loads(str(g["history"]))
    assert len(hist) == 2 and hist[-1]["objective"] == 8582
    _same_rounds(kao, ko, pt, t, g["start"], 2, (g["improved"], hist))


# ---- f. the limit: 2048 nodes ------------------------------------------------------------------------------------------------------
ROWS_F = sorted({64 * b + r for b in range(32) for r in (b, 63 - b)} | {63, 64, 2047})


@pytest.fixture(scope="module")
def limit(kao, ko, kp):
    """The drifted 2040-broker, 7-rack topic (n = np = 2048), its start and the device's 12 dist and 9 mid matrices on it."""
    pt, t = _drifted(ko, 2040, 7, 2400, 3)
    a = _start(kp, t, 1, 2048)
    os.environ.pop(HOOK, None)
    assert kao.cycle_square_plan(2048) == (2048, 1, 2048)
    dev = {(layer, lev): kao.cycle_matrices(pt, a, layer, lev) for layer in range(3) for lev in range(4)}
    return pt, t, a, dev


def test_limit_level_0_matches_the_oracle(kao, ko, limit):
    import kao_cycle as kc
    pt, t, a, dev = limit
    bd = t.bounds()
    assert t.n_brokers + t.n_racks + 1 == 2048 and bd["rack_hi"] != bd["rack_lo"]
    rd = kc.Round(t, a, closures=False)
    B = t.n_brokers
    for layer, E in ((0, rd.EF), (1, rd.ES)):
        d, _, s = dev[layer, 0]
        assert np.array_equal(d, rd._dist0(E)), layer
        assert np.array_equal(s[:B, :B], (E & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:B, :B]), layer
    # L: the oracle's edges on the DEVICE's F closure (its own would take half an hour)
    rd.DF = [dev[0, lev][0].astype(np.int64) for lev in range(4)]
    rd._edges_L()
    d, _, s = dev[2, 0]
    assert np.array_equal(d, rd._dist0L(rd.EL))
    assert np.array_equal(s[:B, :B], (rd.EL & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:B, :B])


def test_limit_priced_l_edges_match_the_oracle_on_the_device_closure(kao, ko, limit):
    """The start of the limit topic has F cycles, so its L layer holds plain replacements only.  After some rounds the F closure
    has no negative diagonal entry: k_cx_transpose runs on 32 x 32 tiles and k_cx_edges_l prices all five variants on the closure
    and its transpose -- compared with the oracle's _edges_L on the device's own closure of that assignment."""
    import kao_cycle as kc
    pt, t, a, dev = limit
    B = t.n_brokers
    assert any((np.diag(dev[0, lev][0])[:B] < 0).any() for lev in (1, 2, 3))
    for rounds in (8, 32, 128):                        # (deterministic: the first of these descents that leaves F without a cycle)
        X = kao.improve_cycles(pt, a, rounds)[0]
        DF = [kao.cycle_matrices(pt, X, 0, lev)[0].astype(np.int64) for lev in range(4)]
        if not any((np.diag(DF[lev])[:B] < 0).any() for lev in (1, 2, 3)):
            break
    else:
        raise AssertionError("F still has a cycle after 128 rounds")
    print("limit topic: F closure without a cycle after", rounds, "rounds")
    rd = kc.Round(t, X, closures=False)
    rd.DF = DF
    assert np.array_equal(rd.DF[0], rd._dist0(rd.EF))
    rd._edges_L()
    d, _, s = kao.cycle_matrices(pt, X, 2, 0)
    assert np.array_equal(d, rd._dist0L(rd.EL))
    assert np.array_equal(s[:B, :B], (rd.EL & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:B, :B])
    variants = set(((rd.EL[rd.EL != np.uint64(kc.NO_EDGE)] >> np.uint64(16)) & np.uint64(15)).tolist())
    assert variants >= {0, 1, 2, 3}, variants          # compensated variants were priced, not only plain replacements


@pytest.mark.parametrize("lev", [1, 2, 3])
@pytest.mark.parametrize("layer", [0, 1, 2])
def test_limit_squarings_row_by_row(limit, layer, lev):
    """Inductively: 66 rows of every squaring -- two in each of the 32 bands of 64 rows, every offset 0..63 within a band (the
    16 x 4 rows a workgroup's lanes own), rows 63, 64 and the global slack node 2047 -- recomputed from the device's previous level
    with the oracle's rule: the smallest sum, the pair's own entry preferred, then the lowest midpoint, clipped at CINF."""
    import kao_cycle as kc
    n = 2048
    assert len({i // 64 for i in ROWS_F}) == 32 and {i % 64 for i in ROWS_F} == set(range(64)) and {0, 63, 64, n - 1} <= set(ROWS_F)
    D = limit[3][layer, lev - 1][0]
    got_d, got_m, _ = limit[3][layer, lev]
    prio = (np.arange(n, dtype=np.int32) + 1)[:, None]
    cols = np.arange(n)
    for i in ROWS_F:
        s = D[i][:, None] + D                          # [k, j]; |sums| <= 2^18, so sum * 4096 + prio fits int32 as it does the device's key
        comp = s * 4096 + prio
        comp[i] = s[i] * 4096
        km = comp.argmin(axis=0)
        assert np.array_equal(got_m[i], km), (layer, lev, i)
        assert np.array_equal(got_d[i], np.minimum(kc.CINF, s[km, cols])), (layer, lev, i)


def test_limit_rounds_stay_feasible_and_beyond_is_refused(kao, ko, limit):
    pt, t, a, _ = limit
    X, obj, st = kao.improve_cycles(pt, a, 2)
    o, v = ko.verify(t, X)
    assert int(np.asarray(v).sum()) == 0 and o == obj == st["objective_after"] >= st["objective_before"] == 17264
    pt2, t2 = _drifted(ko, 2041, 7, 2400, 3)                   # brokers + racks = 2048: one node too many
    with pytest.raises(kao.KaoError) as e:
        kao.improve_cycles(pt2, np.zeros((2400, 3), dtype=np.uint16), 1)
    assert e.value.code == -2                                  # KAO_ERR_UNSUPPORTED
