"""k_search takes three things from small tables or the scalar unit: the penalty (formed with scalar instructions from one packed
scalar), a broker's band row after an accepted move (small-cost form: a per-topic table of five 6-bit entries; a group with a wider
band runs the general form and its arithmetic rows, the host's choice per launch: Session.small_launches() says which ran) and
the row-C7 deltas of a partition's replicas per rack (two 18-bit tables of signed 2-bit fields).  All of it restates the same
arithmetic, so every launch must still replay the scalar restatement (oracle/kao_port.c) bit for bit.

The CPU half (no GPU needed) restates dinc, ddec and band_entry_of and holds the library's own table builders (the hooks
kao_search_band_row / kao_search_rack_delta: band_tab, band_tab_bias, band_tab_fits and c7_tab are the functions the kernels call; the
three instructions that read a table, and the arithmetic form, are device asm and are restated in the hooks -- only the GPU replays
below run the kernels' own) against them exhaustively: every band 0 <= lo <= hi <= 12,
every count 0 .. hi + 3 (the C7 tables hold the counts a partition can have, 0 .. 8, and are walked over those), the arithmetic form
forced as well, and bands one entry too wide for the table, where the arithmetic form is what the hook takes -- and the host,
which then launches the kernel that holds it.  It
also checks that the restatement accepts moves in every GPU case, so the GPU half cannot pass vacuously.

The GPU half replays, per case, three launches against the restatement: final state, best snapshot, best_obj, V, obj, n_accept.
Integer replays: nothing is compared with a tolerance."""
import ctypes as C

import numpy as np
import pytest

from conftest import to_product_topic

LAUNCHES = 3
BAND_MAX = 12
TAB_LAST = 4          # kBandTabLast (kao_search_dev.h): the table holds hi - lo + 3 <= 5 entries


def dinc(c, lo, hi):
    return int(c >= hi) - int(c < lo)


def ddec(c, lo, hi):
    return int(c <= lo) - int(c > hi)


def band_entry_of(c, lo, hi):
    """The six state bits of a band row (kao_search_dev.h): dinc & 3 | (ddec & 3) << 2 | pin << 4 | pout << 5."""
    pin = int(c >= hi or c < lo)
    pout = int(c > hi or c <= lo)
    return (dinc(c, lo, hi) & 3) | ((ddec(c, lo, hi) & 3) << 2) | (pin << 4) | (pout << 5)


@pytest.fixture(scope="module")
def lib():
    from kafka_assignment_optimizer_amd import _ffi
    return _ffi.load()


def test_band_row_lookup_exhaustive(lib):
    """Table and arithmetic form against the restatement for every band and count; the table is used exactly while it fits."""
    fits = C.c_int32(-1)
    n_tab = n_plain = 0
    for lo in range(BAND_MAX + 1):
        for hi in range(lo, BAND_MAX + 1):
            for c in range(hi + 4):
                want = band_entry_of(c, lo, hi)
                assert lib.kao_search_band_row(lo, hi, c, 0, C.byref(fits)) == want, (lo, hi, c)
                assert fits.value == int(hi - lo + 2 <= TAB_LAST), (lo, hi)
                assert lib.kao_search_band_row(lo, hi, c, 1, None) == want, (lo, hi, c, "arithmetic form")
                n_tab += fits.value
                n_plain += 1 - fits.value
    assert n_tab > 0 and n_plain > 0
    # one entry too wide: hi - lo + 3 = 6 entries
    for lo in range(BAND_MAX - 2):
        lib.kao_search_band_row(lo, lo + 3, lo, 0, C.byref(fits))
        assert fits.value == 0
        lib.kao_search_band_row(lo, lo + 2, lo, 0, C.byref(fits))
        assert fits.value == 1


def test_c7_tables_exhaustive(lib):
    """Both bit tables against dinc / ddec for every band and every count a partition can have."""
    seen = set()
    for lo in range(BAND_MAX + 1):
        for hi in range(lo, BAND_MAX + 1):
            for c in range(min(hi + 3, 8) + 1):
                assert lib.kao_search_rack_delta(lo, hi, c, 0) == dinc(c, lo, hi), (lo, hi, c)
                assert lib.kao_search_rack_delta(lo, hi, c, 1) == ddec(c, lo, hi), (lo, hi, c)
                seen |= {dinc(c, lo, hi), ddec(c, lo, hi)}
    assert seen == {-1, 0, 1}


def _tseed(seed, ti):
    return seed ^ (((ti + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


def _oracle_topic(ko, pt):
    return ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                    n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights,
                    bounds_override=dict(pt.bounds_override))


def _case(ko, name):
    """-> dict(ots, restarts, rhos, iters, and optionally prices, team, env; rf3, small: the kernel and key form that must run)"""
    mk = ko.make_cluster
    if name.startswith("p4_"):     # every move kind runs, launches start and end in every phase of the kinds' cycle
        ot = mk("p4", 12, 3, 1, 4, 3, [2, 5], [(12, 2), (13, 0), (14, 1)]).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 1, 4, 7), iters=int(name[3:]), rf3=True, small=True)
    if name.startswith("b40_"):    # restarts turn feasible inside the second or third launch: the penalty leaves lam_max mid-launch and oscillates
        ot = mk("b40", 40, 4, 1, 30, 3, [1, 7, 13], [(40, 2), (41, 3)]).topics[0]   # (the 12-broker shape stays at V = 1 for all its 57 iterations)
        return dict(ots=[ot], restarts=8, rhos=(0, 1, 3, 4, 7), iters=int(name[4:]), rf3=True, small=True)
    if name == "t100_small":       # packed keys with the scalar penalty
        ot = mk("t100", 100, 10, 1, 20, 3, [3, 50, 97], [(100, 0), (101, 4)]).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 7), iters=19, rf3=True, small=True)
    if name == "t100_general":     # general keys with the scalar penalty
        return dict(_case(ko, "t100_small"), small=False, env={"KAO_SEARCH_SMALL": "0"})
    if name == "wide_bands":       # replica band 4 wide (six table entries: the host takes the form with arithmetic rows), partition-rack band [1, 2] (C7 entries other than 0 / 1)
        ot = mk("o3", 30, 3, 1, 20, 3, [4, 17], [(30, 1)], bounds_override={"rep_lo": 1, "rep_hi": 4, "prack_lo": 1, "prack_hi": 2}).topics[0]
        bd = ot.bounds()
        assert (bd["rep_lo"], bd["rep_hi"], bd["prack_lo"], bd["prack_hi"]) == (1, 4, 1, 2)
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 7), iters=19, rf3=True, small=False)   # (costs are small; the bands do not fit a table)
    if name == "prack12":          # the same topic with its own replica band ([2, 2]: a table) -- C7 entries other than 0 / 1 in the small-cost form
        ot = mk("o3n", 30, 3, 1, 20, 3, [4, 17], [(30, 1)], bounds_override={"prack_lo": 1, "prack_hi": 2}).topics[0]
        return dict(ots=[ot], restarts=8, rhos=(0, 3, 7), iters=19, rf3=True, small=True)
    if name in ("rf2", "rf5"):     # the generic kernel, four and eight words per partition
        rf = int(name[2])
        return dict(ots=[mk(name, 90, 6, 1, 40, rf, [4, 31, 77], [(90, 1), (91, 5)]).topics[0]], restarts=8, rhos=(0, 2, 5), iters=19, rf3=False, small=False)
    if name == "priced":
        ots = [mk("b100", 100, 5, 1, 60, 3, [3, 50, 97], [(100, 0), (101, 4)]).topics[0]]
        rng = np.random.default_rng(29)
        prices = [(rng.integers(-8, 9, t.n_brokers).astype(np.int32) * 16384, rng.integers(-4, 5, t.n_brokers).astype(np.int32) * 16384,
                   rng.integers(-2, 3, t.n_racks).astype(np.int32) * 16384) for t in ots]
        return dict(ots=ots, restarts=4, rhos=(0, 3), iters=19, prices=prices, rf3=False, small=False)
    if name == "global":           # one topic in global memory, one wavefront per restart
        from kafka_assignment_optimizer_amd import synthetic as sy
        pts = sy.drift(sy.make_cluster(1000, 20, 1, 6000, 3, [7, 77, 777], [(1000, 7), (1001, 17), (1002, 17)]), 0.2, 3)
        return dict(ots=[_oracle_topic(ko, pts[0])], restarts=3, rhos=(0, 2), iters=19, team=1, env={"KAO_CUR_GLOBAL": "0"}, rf3=False, small=False)
    if name == "team":             # a team of four wavefronts on one restart
        return dict(_case(ko, "global"), team=4, env={})
    raise KeyError(name)


CASES = ["p4_5", "p4_11", "p4_19", "b40_5", "b40_11", "b40_19", "t100_small", "t100_general", "wide_bands", "prack12", "rf2", "rf5", "priced", "global", "team"]
_REFS = {}


def _seed(name):
    return 0x7AB1 + 977 * CASES.index(name)


def _refs(ko, kp, name):
    """The scalar restatement of every (topic, restart) of the case, computed once and shared by both halves."""
    if name not in _REFS:
        case = _case(ko, name)
        out = {}
        for ti, ot in enumerate(case["ots"]):
            for rho in case["rhos"]:
                if case.get("prices") is None:
                    out[(ti, rho)] = kp.port_search(ot, _tseed(_seed(name), ti), rho, LAUNCHES, case["iters"], team=max(1, case.get("team", 0)))
                else:   # (priced launches: the same restatement, launch by launch)
                    run = kp.PortRun(ot, _tseed(_seed(name), ti), rho)
                    for ln in range(LAUNCHES):
                        run.launch(ln, case["iters"], prices=case["prices"][ti])
                    out[(ti, rho)] = run.read()
                    run.close()
        _REFS[name] = (case, out)
    return _REFS[name]


@pytest.mark.parametrize("name", CASES)
def test_restatement_accepts_moves(ko, kp, name):
    """CPU half: kp.port_search accepts moves on every restart of every GPU case."""
    case, refs = _refs(ko, kp, name)
    accepted = {key: ref["n_accept"] for key, ref in refs.items()}
    print(name, "accepted", accepted, "best_obj", {key: ref["best_obj"] for key, ref in refs.items()})
    assert min(accepted.values()) > 0, (name, accepted)
    assert max(accepted.values()) <= LAUNCHES * case["iters"] * max(1, case.get("team", 0))
    if case["rf3"]:
        assert all(ot.rf == 3 and ot.current.shape[1] <= 3 for ot in case["ots"])


def test_restarts_turn_feasible_inside_a_launch(ko, kp):
    """The 40-broker shape: some restart has not been feasible when its second or third launch starts and has when it ends (a launch
    starts from the state the one before ended in, so the snapshot is taken inside the iteration loop and the penalty leaves lam_max
    there), and some restart runs a whole launch with the oscillating penalty."""
    turned = oscillated = 0
    for name in ("b40_5", "b40_11", "b40_19"):
        case, refs = _refs(ko, kp, name)
        ot = case["ots"][0]
        for rho in case["rhos"]:
            b = [kp.port_search(ot, _tseed(_seed(name), 0), rho, n, case["iters"])["best_obj"] for n in range(1, LAUNCHES + 1)]
            assert b[-1] == refs[(0, rho)]["best_obj"]
            turned += int(any(x < 0 <= y for x, y in zip(b[:-1], b[1:])))
            oscillated += int(b[-2] >= 0)
    print("restarts that turned feasible inside a launch", turned, "and ran a later launch feasible", oscillated)
    assert turned > 0 and oscillated > 0


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_tables_replay_bit_exact(kao, ko, kp, monkeypatch, name):
    """GPU half: three launches against the restatement, through the instantiation and key form the case names."""
    case, refs = _refs(ko, kp, name)
    for var in ("KAO_SEARCH_RFT", "KAO_SEARCH_SMALL", "KAO_CUR_GLOBAL"):
        monkeypatch.delenv(var, raising=False)
    for var, val in case.get("env", {}).items():
        monkeypatch.setenv(var, val)
    opts = dict(seed=_seed(name), restarts=case["restarts"], iters_per_launch=case["iters"])
    if "team" in case:
        opts["team"] = case["team"]
    with kao.Session([to_product_topic(t) for t in case["ots"]], **opts) as s:
        if case.get("prices") is not None:
            for ti, pr in enumerate(case["prices"]):
                s.set_prices(ti, *pr)
        s.step(LAUNCHES)
        st = s.stats()
        assert st["drift"] == 0
        assert st["search_rf3_launches"] == (LAUNCHES * st["launch_groups"] if case["rf3"] else 0)
        assert s.small_launches() == (LAUNCHES * st["launch_groups"] if case["small"] else 0)
        devs = {key: s.restart_state(*key) for key in refs}
    for key, dev in devs.items():
        ref = refs[key]
        assert dev["final"].tolist() == ref["final"].tolist(), (name, key)
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (name, key)
        if ref["best_obj"] >= 0:
            assert dev["best"].tolist() == ref["best"].tolist(), (name, key)
