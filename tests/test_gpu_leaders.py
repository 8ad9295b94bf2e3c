"""kao_balance_leaders on the MI355X: the fewest preferred-leader changes that put every broker inside the leader band, replica
sets kept.  Every instance is held against the HiGHS LP of the restricted model (tests/leaders_ref.py
lp_optimum; the matrix is a network matrix, so the LP value is the integer optimum) and against the host restatement of the
kernels' phases, rows and counters bit for bit; every result is checked for the invariants: rows are one swap with slot 0 away
from their input, the violations of C1, C2, C3, C5, C6, C7 do not move, C4 is met, two runs give the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import leaders_ref as lr
from conftest import ROOT

pytestmark = pytest.mark.gpu
STAT_CHECKED = [0, 1, 2, 3, 4, 5, 7]   # everything but the launches, which depend on the regime


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _topic(rows, B, lo, hi, n_racks=2):
    from kafka_assignment_optimizer_amd import Topic
    rows = np.asarray(rows, dtype=np.uint16)
    return Topic(name="t", broker_ids=np.arange(B), rack_of=np.arange(B) % n_racks, n_racks=n_racks, n_partitions=rows.shape[0],
                 rf=rows.shape[1], current=rows, bounds_override={"lead_lo": lo, "lead_hi": hi})


def _checked(kao, topic, opt, model=True):
    """One instance through the GPU, twice; every invariant; n_changed against `opt` (None = infeasible).  Returns the result."""
    from kafka_assignment_optimizer_amd.leaders import balance_leaders
    rows = np.asarray(topic.current, dtype=np.int64)
    res = balance_leaders(topic)
    again = balance_leaders(topic)
    assert res.assignment.tobytes() == again.assignment.tobytes() and res.stats.tolist() == again.stats.tolist()
    assert (res.n_changed, res.status, res.objective) == (again.n_changed, again.status, again.objective)
    obj0, v0 = kao.evaluate(topic, rows)
    obj1, v1 = kao.evaluate(topic, res.assignment)
    print(f"B={topic.n_brokers} P={topic.n_partitions} rf={topic.rf} status={res.status} n_changed={res.n_changed} lp={opt} "
          f"stats={res.stats.tolist()}")
    assert res.objective == obj1
    assert v0[[1, 2, 3, 5, 6, 7]].tolist() == v1[[1, 2, 3, 5, 6, 7]].tolist()
    if opt is None:
        assert res.status == "INFEASIBLE_PROVEN" and res.n_changed == 0 and res.stats[7] > 0
        assert (res.assignment == rows).all()
    else:
        assert res.status == "OPTIMAL_PROVEN" and res.n_changed == opt and res.stats[7] == 0
        assert lr.check_swap(rows, res.assignment) == res.n_changed
        assert v1[4] == 0
        w = topic.weights
        assert obj1 == obj0 - (w[0][0] + w[1][1] - w[0][1] - w[1][0]) * res.n_changed   # no replica moves: 3 per change by default
    if model:
        bd = kao.derive_bounds(topic)
        ok, out, n, stats = lr.kernel_model(rows, topic.n_brokers, bd["lead_lo"], bd["lead_hi"])
        assert (res.assignment == out).all() and n == res.n_changed
        assert [int(res.stats[i]) for i in STAT_CHECKED] == [stats[i] for i in STAT_CHECKED]
    return res


def test_small_family_matches_highs(kao):
    infeasible = 0
    for rows, B, lo, hi in lr.small_family():
        opt = lr.lp_optimum(rows, B, lo, hi)
        infeasible += opt is None
        _checked(kao, _topic(rows, B, lo, hi), opt)
    assert 10 <= infeasible <= 100, infeasible   # both branches are exercised


@pytest.mark.parametrize("seed,B,P", lr.RING_CASES)
def test_ring_family_matches_highs(kao, seed, B, P):
    rows, B, lo, hi = lr.ring_instance(seed, B, P)
    opt = lr.lp_optimum(rows, B, lo, hi)
    assert opt == lr.RING_LP[(seed, B)]
    res = _checked(kao, _topic(rows, B, lo, hi), opt)
    assert res.stats[3] >= 2   # leadership travels over several arcs


# Both sides of the regime choice at the smallest size that reaches it: 65,535 replica slots run in the single workgroup, 65,538 in
# the per-round launches (whose rounds the host settles batch by batch).  HiGHS optimum per case.
@pytest.mark.parametrize("P,optimum,solo", [(21845, 8226, True), (21846, 8530, False)])
def test_regime_threshold_matches_highs_and_the_model(kao, P, optimum, solo):
    rows, B, lo, hi = lr.ring_instance(0, 60, P)
    assert rows.size == 3 * P
    opt = lr.lp_optimum(rows, B, lo, hi)
    assert opt == optimum
    res = _checked(kao, _topic(rows, B, lo, hi), opt, model=True)
    if solo:
        assert res.stats[6] == 1
    else:
        assert res.stats[6] > res.stats[1]   # one launch per round


def _restricted_exact(ko, t):
    """HiGHS on the README model of product topic `t` with every variable of a broker that holds no replica of the partition fixed
    to 0 (one cut row) and the replica, rack and partition-rack bands opened: the model kao_balance_leaders solves."""
    rows = np.asarray(t.current, dtype=np.int64)
    B, P, RF = t.n_brokers, t.n_partitions, t.rf
    ot = ko.Topic(name=t.name, broker_ids=np.array(t.broker_ids), rack_of=np.array(t.rack_of), n_racks=t.n_racks, n_partitions=P, rf=RF,
                  current=rows.astype(np.uint16), weights=t.weights,
                  bounds_override={"rep_lo": 0, "rep_hi": P * RF, "rack_lo": 0, "rack_hi": P * RF, "prack_lo": 0, "prack_hi": RF})
    held = np.zeros((B, P), dtype=bool)
    held[rows, np.arange(P)[:, None]] = True
    coef = np.repeat((~held).astype(float).ravel(), 2)   # variable 2 * (b * P + p) + leader
    return ko.solve_exact(ot, extra_cuts=[(coef, 0, 0)])


def test_config4_matches_highs_and_the_readme_model(kao, ko):
    """BASELINE config 4 after a drift, holes filled: all 200 topics against the flow LP; the first 24 also against HiGHS on the
    README model itself at the default weights, objective by K-eval."""
    topics = lr.config4_topics()
    assert len(topics) == 200
    exact_checked = 0
    for i, t in enumerate(topics):
        rows = np.asarray(t.current, dtype=np.int64)
        bd = kao.derive_bounds(t)
        opt = lr.lp_optimum(rows, t.n_brokers, bd["lead_lo"], bd["lead_hi"])
        res = _checked(kao, t, opt)
        if i < 24:
            ex = _restricted_exact(ko, t)
            if opt is None:
                assert ex.status == "infeasible"
            else:
                assert ex.status == "optimal" and ex.objective == res.objective == kao.evaluate(t, res.assignment)[0], (i, ex.objective, res.objective)
            exact_checked += 1
    assert exact_checked >= 20


def test_large_matches_highs(kao):
    """1000 brokers x 100,000 partitions at RF 3 (the per-round launches): proven, and equal to HiGHS."""
    rows, B, lo, hi = lr.large_instance()
    assert all(len(set(r)) == 3 for r in rows.tolist())
    opt = lr.lp_optimum(rows, B, lo, hi)
    assert opt is not None
    res = _checked(kao, _topic(rows, B, lo, hi, n_racks=10), opt)
    assert res.status == "OPTIMAL_PROVEN" and res.stats[6] > res.stats[1]   # one launch per round


def test_edge_cases(kao):
    # already balanced: nothing to do, no phase
    rows = np.array([[0, 1], [1, 2], [2, 0]])
    res = _checked(kao, _topic(rows, 3, 1, 1), 0)
    assert res.stats[:4].tolist() == [0, 0, 0, 0]
    # one broker leads everything; the only way out runs over two arcs (0 -> 1 -> 2)
    rows = np.array([[0, 1], [0, 1], [1, 2]])
    res = _checked(kao, _topic(rows, 3, 1, 1), lr.lp_optimum(rows, 3, 1, 1))
    assert res.n_changed == 2 and res.stats[3] == 2
    # broker 2 holds no replica at all: lo = 1 cannot be met
    rows = np.array([[0, 1], [1, 0], [0, 1]])
    _checked(kao, _topic(rows, 3, 1, 1), None)
    # an explicit assignment different from topic.current: the objective is measured against current
    from kafka_assignment_optimizer_amd.leaders import balance_leaders
    t = _topic(np.array([[1, 0], [0, 1], [1, 2]]), 3, 1, 1)
    given = np.array([[0, 1], [0, 1], [1, 2]])
    res = balance_leaders(t, given)
    assert res.status == "OPTIMAL_PROVEN" and res.n_changed == 2 and lr.check_swap(given, res.assignment) == 2
    assert (res.assignment == lr.kernel_model(given, 3, 1, 1)[1]).all()
    assert res.objective == kao.evaluate(t, res.assignment)[0]


def test_kao_leaders_cli_end_to_end(kao, tmp_path):
    """cli/kao-leaders on a drifted config 3 cluster: a plan of leader changes only, which kao-waves puts into one wave; the Python
    twin writes the same bytes; --auto-slack reports the slack it needed."""
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
    out_cpp, out_py = tmp_path / "plan_cpp.json", tmp_path / "plan_py.json"
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-leaders")] + base + ["--out", str(out_cpp), "--auto-slack", "--report"], capture_output=True)
    assert r.returncode == 0, r.stderr
    report = r.stderr.decode()
    assert report.count("status=OPTIMAL_PROVEN") == len(topics) and "slack=" in report
    r2 = subprocess.run([sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"] + base + ["--out", str(out_py), "--auto-slack", "--report"],
                        capture_output=True, cwd=ROOT)
    assert r2.returncode == 0, r2.stderr
    assert out_cpp.read_bytes() == out_py.read_bytes() and r2.stderr.decode() == report
    plan = json.loads(out_cpp.read_text())
    before = {(e["topic"], e["partition"]): e["replicas"] for e in cur["partitions"]}
    assert plan["version"] == 1 and plan["partitions"]
    for e in plan["partitions"]:   # changed partitions only, replica sets kept, new leader in front
        old = before[(e["topic"], e["partition"])]
        assert e["replicas"] != old and sorted(e["replicas"]) == sorted(old) and e["replicas"][0] != old[0]
    total = sum(int(line.split("leader_changes=")[1].split()[0]) for line in report.splitlines() if "leader_changes=" in line)
    assert total == len(plan["partitions"])
    w = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", str(cur_path), "--plan", str(out_cpp), "--max-per-broker", "1",
                        "--out-prefix", str(tmp_path / "wave"), "--report"], capture_output=True)
    assert w.returncode == 0, w.stderr
    assert b"waves=1 " in w.stderr
    # without slack a topic whose band cannot be met by leader moves alone is reported, exit status 1
    tight = subprocess.run([os.path.join(ROOT, "cli", "kao-leaders")] + base + ["--out", str(tmp_path / "tight.json"), "--report"], capture_output=True)
    assert tight.returncode in (0, 1)
    assert (tight.returncode == 1) == (b"INFEASIBLE_PROVEN" in tight.stderr)
