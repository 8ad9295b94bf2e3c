"""kao_failover_order on the MI355X: the follower order that keeps the peak leader count after a broker or rack failure as low as it
can be, with the fewest follower swaps.  Every instance goes through `_checked`: two calls give equal bytes,
the five values of every scenario equal the HiGHS reference (tests/failover_ref.py scenario_optimum; the matrix is a network matrix,
so the LP value is the integer optimum), the output rows are the input rows with at most one swap of e(p) and another eligible slot
per row, simulating a failure on them reproduces the reported peaks, a second run on them finds nothing left to do, and a dry run
reports the same numbers on untouched rows."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import failover_ref as fr
from conftest import ROOT

pytestmark = pytest.mark.gpu
NONE = 0xFFFF


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _checked(kao, rows, B, rack_of, R, scope, opt=None):
    from kafka_assignment_optimizer_amd.failover import failover_order_arrays
    rows = np.asarray(rows, dtype=np.int64)
    res = failover_order_arrays(rows, B, rack_of, R, scope)
    again = failover_order_arrays(rows, B, rack_of, R, scope)
    assert res.rows.tobytes() == again.rows.tobytes() and res.scen.tobytes() == again.scen.tobytes()
    assert res.n_reordered == again.n_reordered and res.stats.tolist() == again.stats.tolist()
    if opt is None:
        opt = fr.scenario_optimum(rows, B, rack_of, scope, R)
    print(f"B={B} R={R} P={rows.shape[0]} W={rows.shape[1]} scope={scope} n_reordered={res.n_reordered} stats={res.stats.tolist()}")
    assert res.scen.shape == opt.shape and (res.scen == opt).all(), np.nonzero((res.scen != opt).any(axis=1))[0][:10]
    assert res.n_reordered == int(opt[:, 4].sum())
    assert fr.check_rows(rows, res.rows, B, rack_of, scope) == res.n_reordered
    assert (fr.simulate(res.rows, B, rack_of, scope, R) == opt[:, [0, 1, 3]]).all()
    assert res.stats[0] == int((opt[:, 0] > 0).sum()) and res.stats[7] == int(opt[:, 0].max()) and res.stats[1] >= res.stats[0]
    settled = failover_order_arrays(res.rows, B, rack_of, R, scope)
    assert (settled.scen[:, 4] == 0).all() and settled.n_reordered == 0 and (settled.rows == res.rows).all()
    assert (settled.scen[:, 2] == opt[:, 3]).all() and (settled.scen[:, 3] == opt[:, 3]).all()
    dry = failover_order_arrays(rows, B, rack_of, R, scope, dry_run=True)
    assert (dry.rows == rows).all() and (dry.scen == res.scen).all() and dry.n_reordered == res.n_reordered
    return res


def test_small_family_matches_highs(kao):
    family = fr.small_family()
    assert len(family) == 120
    optima = fr.small_family_optima()
    c = fr.composition(family, optima)
    for kind, floor in fr.COMPOSITION_FLOORS.items():
        assert c[kind] >= floor, (kind, c)
    for (rows, B, rack_of, R), opt in zip(family, optima):
        for scope in (0, 1):
            _checked(kao, rows, B, rack_of, R, scope, opt[scope])


def test_edge_cases(kao):
    # width 1: everything offline, rows untouched
    rows = np.array([[0], [1], [1], [3]])
    res = _checked(kao, rows, 5, np.array([0, 1, 0, 1, 0]), 2, 0)
    assert res.scen[:, 1].tolist() == [1, 2, 0, 1, 0] and res.scen[:, 0].sum() == 0 and (res.rows == rows).all()
    assert res.scen[:, 2].tolist() == [2, 1, 2, 2, 2]   # the survivors' largest leader count
    # RF 2 throughout: no choice
    rng = np.random.default_rng(1)
    rows = np.array([rng.permutation(7)[:2] for _ in range(60)])
    for scope in (0, 1):
        res = _checked(kao, rows, 7, np.arange(7) % 3, 3, scope)
        assert res.n_reordered == 0 and (res.scen[:, 2] == res.scen[:, 3]).all()
    # one rack in rack scope: everything offline, peak 0
    rows = np.array([rng.permutation(6)[:3] for _ in range(20)])
    res = _checked(kao, rows, 6, np.zeros(6, dtype=np.int64), 1, 1)
    assert res.scen.tolist() == [[0, 20, 0, 0, 0]]
    # the only improvement runs over two arcs
    rows, B, rack_of, R = fr.two_arc_instance()
    for scope in (0, 1):
        res = _checked(kao, rows, B, rack_of, R, scope)
        assert res.scen[0].tolist() == [3, 0, 3, 2, 2] and res.stats[5] == 2
        assert res.rows[0].tolist() == [0, 2, 1] and res.rows[1].tolist() == [0, 3, 2]
    # a broker count that is no multiple of 64, partitions on the last broker
    rows, B, rack_of, R = fr.odd_instance()
    assert B % 64 and (rows[:, 0] == B - 1).sum() >= 40
    for scope in (0, 1):
        _checked(kao, rows, B, rack_of, R, scope)


def test_many_workgroups(kao):
    """300 brokers in 10 racks, 9,000 partitions at RF 3: 300 scenarios in broker scope (more than the 256 compute units), 900
    partitions = 2,700 slots per workgroup in rack scope (more than its lanes)."""
    rows, B, rack_of, R = fr.many_instance()
    res = _checked(kao, rows, B, rack_of, R, 0)
    assert res.stats[0] == 300
    res = _checked(kao, rows, B, rack_of, R, 1)
    assert res.stats[0] == 10 and res.stats[7] == 900 and res.n_reordered > 0


def test_broker_limit(kao):
    """An instance at exactly KAO_FAILOVER_MAX_BROKERS brokers, 2,000 partitions at RF 3, broker scope."""
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    limit = int(re.search(r"#define KAO_FAILOVER_MAX_BROKERS (\d+)", header).group(1))
    rows, B, rack_of, R = fr.limit_instance(limit)
    assert B == limit and (rows[:, 0] == B - 1).any()
    res = _checked(kao, rows, B, rack_of, R, 0)
    assert res.stats[0] == 40 and res.n_reordered > 0


def _mixed_topics():
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd import synthetic as sy
    topics = sy.drift(sy.make_config(3, 6), 0.2, 1)
    out = []
    for i, t in enumerate(topics):
        assert t.rf == 3 and not (np.asarray(t.current) == NONE).any()
        if i % 2:
            t = Topic(name=t.name, broker_ids=t.broker_ids, rack_of=t.rack_of, n_racks=t.n_racks, n_partitions=t.n_partitions, rf=2,
                      current=np.asarray(t.current)[:, :2].copy(), weights=t.weights)
        out.append(t)
    return out


def test_mixed_rf_cluster_keeps_objective_and_violations(kao):
    from kafka_assignment_optimizer_amd.failover import failover_order
    topics = _mixed_topics()
    assert {t.rf for t in topics} == {2, 3}
    for scope in ("broker", "rack"):
        plan = failover_order(topics, scope)
        fi = plan.input
        assert fi.rows.shape[1] == 3 and (fi.rows[:, 2] == NONE).any() and not (fi.rows[:, 2] == NONE).all()
        _checked(kao, fi.rows, len(fi.broker_ids), fi.rack_of, topics[0].n_racks, plan.scope)
        assert plan.result.n_reordered == len(plan.entries) > 0
        for t, a in zip(topics, plan.assignments):
            assert a.shape == np.asarray(t.current).shape
            obj0, v0 = kao.evaluate(t, t.current)
            obj1, v1 = kao.evaluate(t, a)
            assert obj0 == obj1 and v0.tolist() == v1.tolist()
            if t.rf == 2:
                assert (a == t.current).all()


def test_kao_failover_cli_end_to_end(kao, tmp_path):
    """cli/kao-failover on a drifted config 3 cluster: a plan of follower swaps only, which kao-waves puts into one wave; the Python
    twin writes the same bytes and the same report."""
    from kafka_assignment_optimizer_amd import assignment_to_json
    from kafka_assignment_optimizer_amd import synthetic as sy
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    topics = sy.drift(sy.make_config(3, 6), 0.2, 1)
    t0 = topics[0]
    cur = assignment_to_json(topics, [t.current for t in topics])
    cur_path, racks_path = tmp_path / "current.json", tmp_path / "racks.json"
    cur_path.write_text(json.dumps(cur))
    racks_path.write_text(json.dumps({str(int(b)): f"r{int(r)}" for b, r in zip(t0.broker_ids, t0.rack_of)}))
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(int(b)) for b in t0.broker_ids), "--racks", str(racks_path)]
    before = {(e["topic"], e["partition"]): e["replicas"] for e in cur["partitions"]}
    for scope in ("broker", "rack"):
        out_cpp, out_py = tmp_path / f"plan_cpp_{scope}.json", tmp_path / f"plan_py_{scope}.json"
        r = subprocess.run([os.path.join(ROOT, "cli", "kao-failover")] + base + ["--scope", scope, "--out", str(out_cpp), "--report"], capture_output=True)
        assert r.returncode == 0, r.stderr
        report = r.stderr.decode()
        r2 = subprocess.run([sys.executable, "-m", "kafka_assignment_optimizer_amd.failover"] + base + ["--scope", scope, "--out", str(out_py), "--report"],
                            capture_output=True, cwd=ROOT)
        assert r2.returncode == 0, r2.stderr
        assert out_cpp.read_bytes() == out_py.read_bytes() and r2.stderr.decode() == report
        plan = json.loads(out_cpp.read_text())
        assert plan["version"] == 1 and plan["partitions"]
        for e in plan["partitions"]:   # reordered partitions only: a permutation with the same first entry
            old = before[(e["topic"], e["partition"])]
            assert e["replicas"] != old and sorted(e["replicas"]) == sorted(old) and e["replicas"][0] == old[0]
        lines = report.splitlines()
        assert lines[-1].startswith(f"scope={scope} ") and all(line.startswith("scenario=") for line in lines[:-1])
        total = int(lines[-1].split(" reordered=")[1])
        assert total == len(plan["partitions"]) == sum(int(line.split(" reordered=")[1]) for line in lines[:-1])
        assert int(lines[-1].split("worst_peak_after=")[1].split()[0]) <= int(lines[-1].split("worst_peak_before=")[1].split()[0])
        w = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", str(cur_path), "--plan", str(out_cpp), "--max-per-broker", "1",
                            "--out-prefix", str(tmp_path / f"wave_{scope}_"), "--report"], capture_output=True)
        assert w.returncode == 0, w.stderr
        assert b"waves=1 " in w.stderr
        dry = subprocess.run([os.path.join(ROOT, "cli", "kao-failover")] + base + ["--scope", scope, "--dry-run", "--report"], capture_output=True)
        assert dry.returncode == 0 and dry.stderr.decode() == report and json.loads(dry.stdout)["partitions"] == []
