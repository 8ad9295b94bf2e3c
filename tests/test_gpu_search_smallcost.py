"""The small-cost form of k_search's RF-3 instantiation.  When the host can show that no move cost of a launch leaves int16
(search_small_cost in kao_search.hip: unpriced and 8 lam_max + 4 obj_scale max|w| <= 16384), the kernel forms its keys as
multiply-adds without the clamp and keeps the two slots of a fused REPLACE scan in the 16-bit halves of one register.  Every launch
must still replay the scalar restatement (oracle/kao_port.c) bit for bit and leave exactly the state the general arithmetic leaves
(KAO_SEARCH_SMALL=0); `Session.small_launches()` says which form ran.

The CPU half (no GPU needed) checks that the restatement accepts moves in every case, so the GPU half cannot pass vacuously, and
checks a Python restatement of the host's rule against a brute-force bound over the row deltas of every move kind.  Integer replays:
nothing is compared with a tolerance."""
import itertools

import pytest

from conftest import to_product_topic

SEED = 0x5C12
RESTARTS = 8
RHOS = (0, 1, 4, 7)
SMALL_COST_MAX = 16384          # kSmallCostMax (kao_internal.h)
DEFAULTS = dict(lam_min=1, lam_max=40, obj_scale=4)   # kao_session.cpp / oracle/kao_port.py DEFAULT_PARAMS
W0 = ((4, 1), (2, 2))           # the default role weights


def small_cost(lam_min, lam_max, obj_scale, w_abs_max, priced=False):
    """search_small_cost (kao_search.hip), restated."""
    if priced or lam_min < 0 or lam_max < lam_min or obj_scale < 1 or w_abs_max < 0:
        return False
    return 8 * lam_max + 4 * obj_scale * w_abs_max <= SMALL_COST_MAX


def _tseed(seed, ti):
    return seed ^ (((ti + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def _shape(ko, name, weights=W0):
    mk = ko.make_cluster
    if name == "p4":         # both slots are often in one partition or share brokers (two brokers leave, three join: with one
        return mk("p4", 12, 3, 1, 4, 3, [2, 5], [(12, 2), (13, 0), (14, 1)], weights=weights).topics[0]   # for one no move is accepted)
    if name == "b40":        # one round: both slots' weighted rounds coincide
        return mk("b40", 40, 4, 1, 30, 3, [1, 7, 13], [(40, 2), (41, 3)], weights=weights).topics[0]
    if name == "b100":       # two rounds: the pair loop meets a weighted round
        return mk("b100", 100, 5, 1, 60, 3, [3, 50, 97], [(100, 0), (101, 4)], weights=weights).topics[0]
    if name == "chain":      # many fused passes: the generator state after each of them
        return mk("chain", 130, 5, 1, 25, 3, [7, 44], [(130, 2)], weights=weights).topics[0]
    if name == "uneven":     # 4 uneven racks: padding indices inside a round
        return mk("uneven", 75, 4, 1, 50, 3, [0, 4, 8, 12, 16, 1], [], weights=weights).topics[0]
    if name == "racks100":   # the rack table is built in two strides
        return mk("racks100", 300, 100, 1, 80, 3, [1, 2, 3], [(300, 1), (301, 2)], weights=weights).topics[0]
    raise KeyError(name)


# name -> (shape, weights, options, launches, iterations per launch, the small-cost form runs)
CASES = {
    "p4": ("p4", W0, {}, 3, 128, True),
    "b40": ("b40", W0, {}, 3, 128, True),
    "b100": ("b100", W0, {}, 3, 128, True),
    "chain": ("chain", W0, {}, 2, 600, True),
    "uneven": ("uneven", W0, {}, 3, 128, True),
    "racks100": ("racks100", W0, {}, 3, 128, True),
    # the largest value of each parameter the rule admits, the others at their defaults: 8 lam_max + 4 S w = 16384 - (0..15)
    "lam_max_admitted": ("b100", W0, dict(lam_max=2040), 3, 128, True),
    "obj_scale_admitted": ("b100", W0, dict(obj_scale=1004), 3, 128, True),
    "weight_admitted": ("b100", ((1004, 1), (2, 2)), {}, 3, 128, True),
    # the smallest the rule refuses
    "lam_max_refused": ("b100", W0, dict(lam_max=2041), 3, 128, False),
    "obj_scale_refused": ("b100", W0, dict(obj_scale=1005), 3, 128, False),
    "weight_refused": ("b100", ((1005, 1), (2, 2)), {}, 3, 128, False),
    # the penalty range kao_solve_capped produces: costs reach the clamp
    "capped": ("b100", W0, dict(lam_max=4000, lam_min=100), 3, 128, False),
}


def _params(opts):
    return dict(DEFAULTS, **opts)


def _wmax(weights):
    return max(abs(w) for row in weights for w in row)


_REFS = {}


def _refs(ko, kp, name):
    """The scalar restatement of every restart of the case, computed once and shared by both halves."""
    if name not in _REFS:
        shape, weights, opts, launches, iters, _ = CASES[name]
        ot = _shape(ko, shape, weights)
        _REFS[name] = (ot, {rho: kp.port_search(ot, _tseed(SEED, 0), rho, launches, iters, **opts) for rho in RHOS})
    return _REFS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_accepts_moves(ko, kp, name):
    """CPU half: the restatement accepts moves on every restart of every case, the rule's restatement says what the case expects,
    and RF 3 with at most 3 current replicas holds (the RF-3 instantiation is the one that runs)."""
    shape, weights, opts, launches, iters, small = CASES[name]
    ot, refs = _refs(ko, kp, name)
    assert ot.rf == 3 and ot.current.shape[1] <= 3
    accepted = [refs[rho]["n_accept"] for rho in RHOS]
    print(name, "accepted per restart", accepted)
    assert min(accepted) > 0, (name, accepted)
    assert max(accepted) <= launches * iters
    pr = _params(opts)
    assert small_cost(pr["lam_min"], pr["lam_max"], pr["obj_scale"], _wmax(weights)) == small


def _brute_force_cost_bound(lam_max, S, weights):
    """The largest |value| the kernel forms: per move kind every combination of row deltas in {-1, 0, +1} over the rows the kind
    touches and every combination of role weights (or none) in the objective terms; for the scans also the constant K0 and the sum
    K0 + lam dVx - S w.  The penalty lam is at most lam_max and every expression is linear in it, so lam_max gives the extremes."""
    ws = sorted({0} | {w for row in weights for w in row})
    worst = 0

    def sums(rows):
        return range(-rows, rows + 1)   # every sum of `rows` deltas in {-1, 0, 1}

    lam = lam_max
    for dV in sums(8):                   # REPLACE: 2 replica rows, 2 leader rows, 2 rack totals, 2 partition-rack counts
        for new, old in itertools.product(ws, ws):
            worst = max(worst, abs(lam * dV - S * (new - old)))
    for dV in sums(6):                   # EXCHANGE: 2 leader rows, 4 partition-rack counts; four role weights
        for a, b, c, d in itertools.product(ws, repeat=4):
            worst = max(worst, abs(lam * dV - S * (a + b - c - d)))
    for dV in sums(2):                   # LEADER-SWAP: 2 leader rows; four role weights
        for a, b, c, d in itertools.product(ws, repeat=4):
            worst = max(worst, abs(lam * dV - S * (a + b - c - d)))
    for sc in sums(4):                   # tournament score of a slot: lam sc + S g
        for g in ws:
            worst = max(worst, abs(lam * sc + S * g))
    for dV_old in sums(2):               # scans: K0 = S g_old + lam dV_old, then K0 + lam dVx - S w with 6 rows in dVx
        for g in ws:
            k0 = S * g + lam * dV_old
            worst = max(worst, abs(k0))
            for dVx in sums(6):
                for w in ws:
                    worst = max(worst, abs(k0 + lam * dVx - S * w), abs(lam * dVx))
    return worst


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][2] or CASES[n][1] != W0] + ["b100"])
def test_rule_against_brute_force(name):
    """The rule's quantity 8 lam_max + 4 S w bounds every value the kernel forms; what the rule admits stays within half of int16's
    range (so the biased cost field is far from 0, from the clamp's upper end 65534 and from the no-candidate value 65535), and what
    it refuses here is refused by that margin or because it can truly leave int16."""
    _, weights, opts, _, _, small = CASES[name]
    pr = _params(opts)
    w = _wmax(weights)
    worst = _brute_force_cost_bound(pr["lam_max"], pr["obj_scale"], weights)
    rule = 8 * pr["lam_max"] + 4 * pr["obj_scale"] * w
    print(name, "brute-force bound", worst, "rule quantity", rule)
    assert worst <= rule
    assert small_cost(pr["lam_min"], pr["lam_max"], pr["obj_scale"], w) == small == (rule <= SMALL_COST_MAX)
    if small:
        assert worst <= SMALL_COST_MAX and 32768 + worst < 65534 and 32768 - worst > 0
    assert not small_cost(pr["lam_min"], pr["lam_max"], pr["obj_scale"], w, priced=True)


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _run(kao, ot, launches, iters, opts):
    with kao.Session([to_product_topic(ot)], seed=SEED, restarts=RESTARTS, iters_per_launch=iters, **opts) as s:
        s.step(launches)
        st = s.stats()
        assert st["drift"] == 0
        states = {rho: s.restart_state(0, rho) for rho in RHOS}
        return states, s.best_keys().tolist(), st, s.small_launches()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_small_cost_replays_and_matches_general(kao, ko, kp, monkeypatch, name):
    """GPU half: bit-exact replay through the form the rule picks, the getter says which one ran, and the same session with
    KAO_SEARCH_SMALL=0 leaves byte-identical restart states and best keys."""
    _, _, opts, launches, iters, small = CASES[name]
    ot, refs = _refs(ko, kp, name)
    for var in ("KAO_SEARCH_RFT", "KAO_SEARCH_SMALL"):
        monkeypatch.delenv(var, raising=False)
    states, keys, st, n_small = _run(kao, ot, launches, iters, opts)
    assert st["search_rf3_launches"] == launches * st["launch_groups"]
    assert n_small == (launches * st["launch_groups"] if small else 0)
    for rho, dev in states.items():
        ref = refs[rho]
        assert dev["final"].tolist() == ref["final"].tolist(), (name, rho)
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (name, rho)
        if ref["best_obj"] >= 0:
            assert dev["best"].tolist() == ref["best"].tolist(), (name, rho)
    monkeypatch.setenv("KAO_SEARCH_SMALL", "0")
    states0, keys0, st0, n_small0 = _run(kao, ot, launches, iters, opts)
    assert st0["search_rf3_launches"] == launches * st0["launch_groups"] and n_small0 == 0
    for rho in RHOS:
        x, y = states[rho], states0[rho]
        assert x["final"].tobytes() == y["final"].tobytes(), (name, rho)
        assert x["best"].tobytes() == y["best"].tobytes(), (name, rho)
        assert (x["best_obj"], x["V"], x["obj"], x["n_accept"]) == (y["best_obj"], y["V"], y["obj"], y["n_accept"]), (name, rho)
    assert keys == keys0
