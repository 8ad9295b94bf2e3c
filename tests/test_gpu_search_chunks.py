"""K-search as ticketed chunks (kao_search.hip: chunk_take / chunk_pass; kao_session.cpp: plan_chunks; KAO_SEARCH_CHUNKS): a launch
of n iterations runs, per block-map entry, as C shorter pieces inside one grid.  A later piece is the launch carried on -- the packed
state, restart_info and every lane's generator word handed over through global memory behind a release / acquire pair at agent scope
-- so the result is that of the launch in one piece, bit for bit.

Every case runs three launches with KAO_SEARCH_CHUNKS forced, is replayed against oracle/kao_port.c (state, snapshot, best_obj, V,
obj, n_accept) and compared byte for byte, every restart, with the same session under KAO_SEARCH_CHUNKS=1; drift stays 0.  The cases
are the smallest shapes where the hand-off can go wrong: uneven splits (19 = 5 + 5 + 5 + 4), a plan that has to shrink (5 iterations,
8 chunks asked for), one entry whose four workgroups start together (three really wait), a workgroup with a wavefront that has no
restart, restarts that turn feasible in a later chunk (best_obj, the sawtooth penalty and a snapshot cross a boundary: the CPU half
asserts it), an elite launch, the generic instantiations, and more entries than the device holds at once.  Topics in global memory
and teams must launch in one piece."""
import numpy as np
import pytest

import test_gpu_search_chains as chains
from conftest import to_product_topic

LAUNCHES = 3
HOOK = "KAO_SEARCH_CHUNKS"
_ENV_VARS = chains._ENV_VARS + (HOOK,)

# name -> (case of tests/test_gpu_search_chains.py, overrides, iterations per launch, chunks forced, chunks the plan must give)
CASES = {
    "split_19_by_4": ("one_round", {}, 19, 4, 4),
    "split_11_by_2": ("one_round", {}, 11, 2, 2),
    "split_5_by_8_shrinks": ("one_round", {}, 5, 8, 5),
    "one_entry_three_wait": ("one_round", dict(restarts=4, rhos=(0, 1, 2, 3)), 19, 4, 4),
    "wavefront_without_restart": ("one_round", dict(restarts=7, rhos=(0, 3, 4, 6)), 19, 4, 4),
    "moves_of_every_kind": ("moves_of_every_kind", {}, 19, 4, 4),
    "rf2": ("rf2", {}, 19, 4, 4),
    "rf5": ("rf5", {}, 19, 4, 4),
    "general_cost": ("two_rounds_general", {}, 19, 4, 4),
    "priced_broker_weights": ("priced_broker_weights", {}, 19, 4, 4),
    "wide_topic": ("wide", {}, 19, 4, 4),
    "global_memory": ("global_memory", {}, 19, 4, 0),
    "team_of_four": ("team_of_four", {}, 19, 4, 0),
}
_BUILT = {}


def _case(ko, name):
    if name not in _BUILT:
        base, over, iters, forced, chunks = CASES[name]
        if base == "wide":   # 100 brokers / 5 racks / 180 partitions: 540 replica slots, the wide instantiation, two rounds per scan
            ot = chains._drifted(ko, 100, 5, 180, 3, [3, 50], [], 0.2, 5)
            case = dict(ots=[ot], restarts=8, rhos=(0, 5, 7), rf3=True, small=True, seed=0xC4A17 + 811 * 101)
        else:
            case = dict(chains._case(ko, base), seed=chains._seed(base), **over)
        _BUILT[name] = dict(case, iters=iters, forced=forced, chunks=chunks)
    return _BUILT[name]


def _seed(case):
    return case["seed"]


def _replay(kp, case, ti, ot, rho, launches, iters):
    """tests/test_gpu_search_chains.py::_replay with this case's seed"""
    team = max(1, case.get("team", 0))
    if case.get("prices") is None:
        return kp.port_search(ot, chains._tseed(_seed(case), ti), rho, launches, iters, team=team)
    run = kp.PortRun(ot, chains._tseed(_seed(case), ti), rho)
    for ln in range(launches):
        run.launch(ln, iters, prices=case["prices"][ti])
    out = run.read()
    run.close()
    return out


def _state_tuple(dev):
    return (dev["final"].tobytes(), dev["best"].tobytes(), dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"])


def _run(kao, monkeypatch, case, hook, topics=None, restarts=None, which=None):
    """One session, three launches -> (state of every listed (topic, restart), best keys, stats, chunked launches)"""
    for var in _ENV_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in case.get("env", {}).items():
        monkeypatch.setenv(var, val)
    if hook is not None:   # (None: the variable unset -- the automatic rule)
        monkeypatch.setenv(HOOK, str(hook))
    ots = topics if topics is not None else case["ots"]
    n_restarts = restarts if restarts is not None else case["restarts"]
    opts = dict(seed=_seed(case), restarts=n_restarts, iters_per_launch=case["iters"])
    if "team" in case:
        opts["team"] = case["team"]
    with kao.Session([to_product_topic(t) for t in ots], **opts) as s:
        if case.get("prices") is not None:
            for ti, pr in enumerate(case["prices"]):
                s.set_prices(ti, *pr)
        s.step(LAUNCHES)
        st = s.stats()
        keys = s.best_keys().tolist()
        pairs = which if which is not None else [(ti, rho) for ti in range(len(ots)) for rho in range(n_restarts)]
        states = {key: s.restart_state(*key) for key in pairs}
        return states, keys, st, s.chunked_launches()


def test_feasibility_crosses_a_chunk_boundary(ko, kp):
    """CPU half: in moves_of_every_kind at 19 iterations in chunks of 5, 5, 5, 4, some restart of the first launch is infeasible at
    the end of the first chunk and feasible later (best_obj and, with it, the sawtooth penalty change in a later chunk and are carried
    over further boundaries), and some snapshot is taken in a chunk behind the first."""
    case = _case(ko, "moves_of_every_kind")
    ot = case["ots"][0]
    bounds = (5, 10, 15)
    late_feasible = late_snapshot = carried = 0
    for rho in case["rhos"]:
        objs = [_replay(kp, case, 0, ot, rho, 1, i)["best_obj"] for i in range(case["iters"] + 1)]   # a launch of i iterations is the first i of a longer one
        turn = next((i for i in range(1, len(objs)) if objs[i - 1] < 0 <= objs[i]), None)
        late_feasible += turn is not None and turn > bounds[0]
        carried += turn is not None and turn <= bounds[-1]
        late_snapshot += any(objs[i] != objs[i - 1] for i in range(bounds[0] + 1, len(objs)))
    print("feasible in a later chunk", late_feasible, "| feasible with a boundary still ahead", carried, "| snapshot in a later chunk", late_snapshot)
    assert late_feasible >= 1 and carried >= 1 and late_snapshot >= 1


def test_cases_are_what_they_claim(ko):
    """CPU half: block-map entries (four restarts per workgroup) and slots per case, from the shapes alone."""
    assert _case(ko, "one_entry_three_wait")["restarts"] <= 4                       # one block-map entry
    assert _case(ko, "wavefront_without_restart")["restarts"] % 4 == 3              # the last workgroup: three restarts, four wavefronts
    wide = _case(ko, "wide_topic")["ots"][0]
    assert wide.n_partitions * wide.rf >= 512
    import kafka_assignment_optimizer_amd as kao
    for name, (_, _, iters, forced, chunks) in CASES.items():
        if chunks:
            entries = -(-_case(ko, name)["restarts"] // 4)
            assert len(kao.search_chunk_plan(entries, 1536, iters, forced)) == entries * chunks, name


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_chunked_launches_replay_bit_exact(kao, ko, kp, monkeypatch, name):
    case = _case(ko, name)
    chunked, keys_c, st_c, n_c = _run(kao, monkeypatch, case, case["forced"])
    whole, keys_w, st_w, n_w = _run(kao, monkeypatch, case, 1)
    assert st_c["drift"] == 0 and st_w["drift"] == 0
    assert n_w == 0
    assert n_c == (LAUNCHES * st_c["launch_groups"] if case["chunks"] else 0), (name, n_c)   # (global memory, teams: in one piece)
    assert keys_c == keys_w, name
    for key in whole:
        assert _state_tuple(chunked[key]) == _state_tuple(whole[key]), (name, key)
    for ti, ot in enumerate(case["ots"]):
        for rho in case["rhos"]:
            ref, dev = _replay(kp, case, ti, ot, rho, LAUNCHES, case["iters"]), chunked[(ti, rho)]
            assert dev["final"].tolist() == ref["final"].tolist(), (name, ti, rho)
            assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (name, ti, rho)
            if ref["best_obj"] >= 0:
                assert dev["best"].tolist() == ref["best"].tolist(), (name, ti, rho)


@pytest.mark.gpu
def test_more_entries_than_the_device_holds(kao, ko, kp, monkeypatch):
    """Six copies of the 12-broker topic x 1,536 restarts: 2,304 block-map entries, 9,216 tickets at C = 4 -- more workgroups than are
    resident at once, so later chunks are taken while other entries' first chunks still wait for a slot.  Every restart against the
    launch in one piece, a handful against the restatement; and the automatic rule leaves these 19-iteration launches in one piece."""
    case = dict(_case(ko, "split_19_by_4"))
    ots = [case["ots"][0]] * 6
    restarts = 1536
    chunked, keys_c, st_c, n_c = _run(kao, monkeypatch, case, 4, topics=ots, restarts=restarts)
    whole, keys_w, st_w, n_w = _run(kao, monkeypatch, case, 1, topics=ots, restarts=restarts)
    assert st_c["drift"] == 0 and st_w["drift"] == 0 and st_c["blocks_search"] == 2304
    assert n_c == LAUNCHES * st_c["launch_groups"] and n_w == 0
    assert keys_c == keys_w
    assert len(whole) == 6 * restarts
    for key in whole:
        assert _state_tuple(chunked[key]) == _state_tuple(whole[key]), key
    for ti, rho in ((0, 0), (2, 777), (5, 1535), (3, 1021)):
        ref, dev = _replay(kp, case, ti, ots[ti], rho, LAUNCHES, case["iters"]), chunked[(ti, rho)]
        assert dev["final"].tolist() == ref["final"].tolist(), (ti, rho)
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (ti, rho)
    _, keys_a, _, n_a = _run(kao, monkeypatch, case, 0, topics=ots, restarts=restarts, which=[(0, 0)])
    assert n_a == 0 and keys_a == keys_w


@pytest.mark.gpu
def test_automatic_rule_chunks_the_tail_only(kao, ko, kp, monkeypatch):
    """The shape that ships as the default, with KAO_SEARCH_CHUNKS unset: 3,456 entries (2.25 resident rounds) at 128 iterations per launch.  One
    grid mixes the entries in front of the tail, in one piece, with the last resident round of entries in two chunks of 64 iterations
    (four would fall below 64).  Every restart against the launch in one piece, a handful against the restatement."""
    case = dict(_case(ko, "split_19_by_4"), iters=128)
    ots = [case["ots"][0]] * 6
    restarts = 2304
    auto, keys_a, st_a, n_a = _run(kao, monkeypatch, case, None, topics=ots, restarts=restarts)
    whole, keys_w, st_w, n_w = _run(kao, monkeypatch, case, 1, topics=ots, restarts=restarts)
    assert st_a["drift"] == 0 and st_w["drift"] == 0 and st_a["blocks_search"] == 3456
    assert n_a == LAUNCHES * st_a["launch_groups"] and n_w == 0
    assert keys_a == keys_w
    for key in whole:
        assert _state_tuple(auto[key]) == _state_tuple(whole[key]), key
    for ti, rho in ((0, 0), (1, 300), (3, 1021), (5, 2303)):
        ref, dev = _replay(kp, case, ti, ots[ti], rho, LAUNCHES, case["iters"]), auto[(ti, rho)]
        assert dev["final"].tolist() == ref["final"].tolist(), (ti, rho)
        assert (dev["best_obj"], dev["V"], dev["obj"], dev["n_accept"]) == (ref["best_obj"], ref["V"], ref["obj"], ref["n_accept"]), (ti, rho)
    # the rule covers the small-cost RF-3 kernel only: the same batch with the general cost arithmetic launches in one piece
    general = dict(case, env={"KAO_SEARCH_SMALL": "0"})
    _, keys_g, st_g, n_g = _run(kao, monkeypatch, general, None, topics=ots, restarts=restarts, which=[(0, 0)])
    assert n_g == 0 and st_g["drift"] == 0 and keys_g == keys_w


@pytest.mark.gpu
def test_elite_launch_chunked(kao, ko, kp, monkeypatch):
    """An elite launch as the third launch (elite_period = 2), in four chunks: the first chunk applies the re-seeding rule, the later
    ones must not (they would re-seed a second time).  Against the restatement and against the launch in one piece."""
    import test_gpu_parity as parity
    ots = parity._drifted(ko, 4, 3)
    pts = [to_product_topic(t) for t in ots]
    seed, iters, restarts = 4242, 120, 16
    out = {}
    for hook in (4, 1):
        for var in _ENV_VARS:
            monkeypatch.delenv(var, raising=False)
        monkeypatch.setenv(HOOK, str(hook))
        with kao.Session(pts, seed=seed, restarts=restarts, iters_per_launch=iters, elite_period=2) as s:
            s.step(2)
            res = s.best()                 # what launch 2 (an elite launch) re-seeds from
            s.step(1)
            assert s.stats()["drift"] == 0
            assert s.chunked_launches() == (3 * s.stats()["launch_groups"] if hook == 4 else 0)
            out[hook] = (res, {(ti, rho): s.restart_state(ti, rho) for ti in range(len(ots)) for rho in range(restarts)}, s.best_keys().tolist())
    assert out[4][2] == out[1][2]
    for key in out[1][1]:
        assert _state_tuple(out[4][1][key]) == _state_tuple(out[1][1][key]), key
    res, states, _ = out[4]
    reseeded = 0
    for ti, ot in enumerate(ots):
        r = res[ti]
        assert r.status != "NO_FEASIBLE"
        for rho in range(restarts):
            run = kp.PortRun(ot, parity._tseed(seed, ti), rho)
            run.launch(0, iters)
            run.launch(1, iters)
            before = run.read()
            run.launch(2, iters, elite=(r.assignment, r.objective, r.best_restart))
            ref = run.read()
            run.close()
            dev = states[(ti, rho)]
            assert dev["final"].tolist() == ref["final"].tolist(), (ti, rho)
            assert (dev["best_obj"], dev["V"], dev["obj"]) == (ref["best_obj"], ref["V"], ref["obj"])
            reseeded += before["best_obj"] < r.objective and ref["best_obj"] >= r.objective
    assert reseeded > 0            # the rule fired somewhere
