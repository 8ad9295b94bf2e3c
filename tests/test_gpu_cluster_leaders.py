"""kao_balance_leaders_cluster on the MI355X: the preferred leaders of all topics chosen together so that every topic's band holds
and the cluster-wide peak is as low as leader changes alone can make it, with the fewest changes.  Every
instance is held against the HiGHS LP of the definition (tests/cluster_leaders_ref.py; a network matrix, so the LP value is the
integer optimum); every result is checked for the invariants: rows are one swap with slot 0 away from their input, every band
holds, n_changed is the number of rows that differ, two calls give the same bytes, dry_run reports the same numbers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_leaders_ref as cr
import leaders_ref as lr
from conftest import ROOT

pytestmark = pytest.mark.gpu
NONE = 0xFFFF


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def call(kao):
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_cluster_arrays
    return balance_leaders_cluster_arrays


def _numbers(res):
    return res.status, res.n_changed, res.peak_before, res.peak_after


def _checked(call, rows, topic_of, B, LO, tlo, thi, cluster_hi=-1):
    """One instance through the GPU: twice, and once with dry_run; every invariant.  Returns the result."""
    rows = np.asarray(rows, dtype=np.int64)
    res = call(rows, B, topic_of, tlo, thi, LO, cluster_hi)
    again = call(rows, B, topic_of, tlo, thi, LO, cluster_hi)
    dry = call(rows, B, topic_of, tlo, thi, LO, cluster_hi, dry_run=True)
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all()
    assert res.peak_before == (int(np.bincount(rows[:, 0], minlength=B).max()) if len(rows) else 0)
    if res.status == "OPTIMAL_PROVEN":
        assert cr.check_rows(rows, res.rows) == res.n_changed == int((res.rows != rows).any(axis=1).sum())
        assert cr.admissible(res.rows, topic_of, B, LO, res.peak_after, tlo, thi)
        assert res.peak_after == (int(np.bincount(res.rows[:, 0].astype(np.int64), minlength=B).max()) if len(rows) else 0)
        assert res.stats[7] == 0
    else:
        assert res.status == "INFEASIBLE_PROVEN" and res.n_changed == 0 and res.peak_after == res.peak_before and (res.rows == rows).all()
    return res


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_matches_highs(call):
    feasible = 0
    for seed in range(80):
        rows, topic_of, B, LO, tlo, thi = cr.small_case(seed)
        opt = cr.optimum(rows, topic_of, B, LO, tlo, thi)
        res = _checked(call, rows, topic_of, B, LO, tlo, thi)
        print(f"seed={seed} B={B} P={len(rows)} T={len(tlo)} lo={LO} opt={opt} gpu={_numbers(res)} stats={res.stats.tolist()}")
        if opt is None:
            assert res.status == "INFEASIBLE_PROVEN", seed
            continue
        feasible += 1
        peak, n = opt
        assert res.status == "OPTIMAL_PROVEN" and (res.peak_after, res.n_changed) == (peak, n), seed
        above = _checked(call, rows, topic_of, B, LO, tlo, thi, cluster_hi=peak + 1)
        assert above.status == "OPTIMAL_PROVEN" and above.n_changed == cr.lp(rows, topic_of, B, LO, peak + 1, tlo, thi), seed
        assert above.peak_after <= peak + 1, seed
        if peak - 1 >= LO:
            assert _checked(call, rows, topic_of, B, LO, tlo, thi, cluster_hi=peak - 1).status == "INFEASIBLE_PROVEN", seed
    assert feasible >= 50


# ---- 2. one topic reduces to section 4h ----------------------------------------------------------------------------------------------
def _one_topic_cases():
    out = [("ring",) + lr.ring_instance(0, 60, 1800)]
    feasible = infeasible = 0
    for i, (rows, B, lo, hi) in enumerate(lr.small_family()):   # eight that can be balanced and two that cannot
        ok = lr.lp_optimum(rows, B, lo, hi) is not None
        if (feasible < 8) if ok else (infeasible < 2):
            out.append((f"small{i}", rows, B, lo, hi))
            feasible, infeasible = feasible + ok, infeasible + (not ok)
        if feasible == 8 and infeasible == 2:
            break
    return out


def test_one_topic_reduces_to_balance_leaders(kao, call):
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders
    cases = _one_topic_cases()
    assert len(cases) == 11
    for name, rows, B, lo, hi in cases:
        P = len(rows)
        t = Topic(name="t", broker_ids=np.arange(B), rack_of=np.arange(B) % 2, n_racks=2, n_partitions=P, rf=rows.shape[1],
                  current=rows.astype(np.uint16), bounds_override={"lead_lo": lo, "lead_hi": hi})
        one = balance_leaders(t)
        res = _checked(call, rows, np.zeros(P, dtype=np.int32), B, lo, [0], [P], cluster_hi=hi)
        print(f"{name}: 4h={one.status, one.n_changed} cluster={_numbers(res)}")
        assert res.status == one.status and res.n_changed == one.n_changed, name
        if name == "ring":
            assert res.n_changed == 700


# ---- 3. the mid instance -------------------------------------------------------------------------------------------------------------
def test_mid_instance_matches_highs(call):
    """mid_case(100, 20, 150, 3, 0), topic bands [0, 3]: the result against the two LPs around its peak (the reference says 75 -> 30
    with 406 changes; with bands [0, 3000] it is 346, so the topic bands bind)."""
    rows, topic_of = cr.mid_case(100, 20, 150, 3, 0)
    tlo, thi = np.zeros(20, dtype=np.int64), np.full(20, 3)
    res = _checked(call, rows, topic_of, 100, 0, tlo, thi)
    print(f"mid: {_numbers(res)} stats={res.stats.tolist()}")
    assert res.status == "OPTIMAL_PROVEN"
    assert cr.lp(rows, topic_of, 100, 0, res.peak_after - 1, tlo, thi) is None
    assert cr.lp(rows, topic_of, 100, 0, res.peak_after, tlo, thi) == res.n_changed
    assert res.stats[5] > 1   # the multi-launch path ran


# ---- 4. config 4 concatenated --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config4():
    topics = lr.config4_topics()
    rows = np.concatenate([np.asarray(t.current, dtype=np.int64) for t in topics])
    topic_of = np.repeat(np.arange(len(topics)), [t.n_partitions for t in topics])
    return topics, rows, topic_of


@pytest.mark.parametrize("cluster_lo", [0, 7])
def test_config4_matches_highs_and_keeps_every_topic_valid(kao, call, config4, cluster_lo):
    """200 topics x 50 partitions on 500 brokers, bands [0, 1] (measured with HiGHS: 148 -> 40 with 5,340 changes, 5,343 at
    cluster_lo = 7): the result against the two LPs around its peak, C4 of every topic by K-eval, replica sets kept."""
    topics, rows, topic_of = config4
    B, T = topics[0].n_brokers, len(topics)
    tlo, thi = np.zeros(T, dtype=np.int64), np.ones(T, dtype=np.int64)
    res = _checked(call, rows, topic_of, B, cluster_lo, tlo, thi)
    print(f"config 4, cluster_lo={cluster_lo}: {_numbers(res)} stats={res.stats.tolist()}")
    assert res.status == "OPTIMAL_PROVEN"
    assert cr.lp(rows, topic_of, B, cluster_lo, res.peak_after - 1, tlo, thi) is None
    assert cr.lp(rows, topic_of, B, cluster_lo, res.peak_after, tlo, thi) == res.n_changed
    assert (np.sort(res.rows.astype(np.int64), axis=1) == np.sort(rows, axis=1)).all()
    at = 0
    for t in topics:
        assert kao.evaluate(t, res.rows[at:at + t.n_partitions])[1][4] == 0, t.name
        at += t.n_partitions


def test_config4_floor_above_the_feasible_one_is_infeasible(call, config4):
    topics, rows, topic_of = config4
    T = len(topics)
    res = _checked(call, rows, topic_of, topics[0].n_brokers, 8, np.zeros(T, dtype=np.int64), np.ones(T, dtype=np.int64))
    assert res.status == "INFEASIBLE_PROVEN" and res.stats[7] > 0


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------
def test_edge_cases(call):
    # no partition at all
    res = _checked(call, np.zeros((0, 3)), np.zeros(0), 4, 0, [0], [1])
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0)
    assert _checked(call, np.zeros((0, 3)), np.zeros(0), 4, 1, [0], [1]).status == "INFEASIBLE_PROVEN"
    # width 1: nothing to choose, feasible exactly when the input is admissible
    rows, topic_of = np.array([[0], [1], [0], [2]]), np.array([0, 0, 1, 1])
    res = _checked(call, rows, topic_of, 3, 0, [0, 0], [1, 1])
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 2, 2)
    assert _checked(call, rows, topic_of, 3, 1, [0, 0], [1, 1]).status == "OPTIMAL_PROVEN"
    assert _checked(call, rows, topic_of, 3, 2, [0, 0], [1, 1]).status == "INFEASIBLE_PROVEN"       # brokers 1 and 2 lead one each
    assert _checked(call, rows, topic_of, 3, 0, [0, 0], [1, 1], cluster_hi=1).status == "INFEASIBLE_PROVEN"   # broker 0 leads two
    assert _checked(call, np.array([[0], [0]]), np.array([0, 0]), 2, 0, [0], [1]).status == "INFEASIBLE_PROVEN"   # two of topic 0 on broker 0
    # topic_lo = 1 where broker 2 holds no replica of topic 0: infeasible, rows untouched
    rows, topic_of = np.array([[0, 1], [1, 0], [2, 0], [1, 2]]), np.array([0, 0, 1, 1])
    assert _checked(call, rows, topic_of, 3, 0, [1, 0], [2, 2]).status == "INFEASIBLE_PROVEN"
    assert _checked(call, rows, topic_of, 3, 0, [0, 0], [2, 2]).status == "OPTIMAL_PROVEN"
    # the input breaks a topic band: the peak has to rise (broker 0 may lead one partition of the topic, broker 1 takes the other)
    rows = np.array([[0, 1], [0, 1], [1, NONE]])
    res = _checked(call, rows, np.array([0, 0, 1]), 2, 0, [0, 0], [1, 1])
    assert _numbers(res) == ("OPTIMAL_PROVEN", 1, 2, 2) and cr.optimum(rows, [0, 0, 1], 2, 0, [0, 0], [1, 1]) == (2, 1)


def test_invalid_arguments_leave_the_rows_alone(kao):
    """Every invalid argument of include/kao.h gives KAO_ERR_INVALID on a machine with a device too."""
    import test_cluster_leaders_ref as host
    for what, change in host.INVALID:
        kw = dict(rows=[[0, 1], [2, 3], [1, 2]], B=4, topic_of=[0, 0, 1], tlo=[0, 0], thi=[1, 1])
        kw.update(change)
        assert host._call(**kw) == -1, what   # (_call asserts that the row buffer is unchanged)


# ---- 6. the command-line tools -------------------------------------------------------------------------------------------------------
def test_cli_cluster_end_to_end(kao, tmp_path):
    """cli/kao-leaders --cluster and its Python twin on a three-topic document of mixed RF: the same bytes, a plan of the changed rows
    only, which applied to the document gives the library's rows."""
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_cluster_arrays
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(7)
    B, ids = 8, [100 + 3 * i for i in range(8)]
    doc = {"version": 1, "partitions": []}
    for name, P, rf in (("alpha", 12, 3), ("beta", 9, 2), ("gamma", 7, 1)):
        for p in range(P):
            r = rng.permutation(B)[:rf]
            if rng.random() < 0.7 and (r < 2).any():   # brokers 0 and 1 lead what they hold
                j = int(np.nonzero(r < 2)[0][0])
                r[[0, j]] = r[[j, 0]]
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
    cur_path, racks_path = tmp_path / "current.json", tmp_path / "racks.json"
    cur_path.write_text(json.dumps(doc))
    racks_path.write_text(json.dumps({str(b): f"r{i % 2}" for i, b in enumerate(ids)}))
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path)]
    progs = ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"])
    outs = []
    for i, prog in enumerate(progs):
        out = tmp_path / f"plan{i}.json"
        r = subprocess.run(prog + base + ["--cluster", "--report", "--slack", "1", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append((out.read_bytes(), r.stderr.decode()))
        assert subprocess.run(prog + base + ["--cluster", "--auto-slack"], capture_output=True, cwd=ROOT).returncode == 2
    assert outs[0] == outs[1]
    report = outs[0][1].splitlines()
    assert len(report) == 1 and report[0].startswith("cluster: status=OPTIMAL_PROVEN peak_before=")
    # the library on the same rows: partitions ordered by (topic, partition), bands floor / ceil widened by the slack
    from kafka_assignment_optimizer_amd.failover import parse_current
    fi = parse_current(doc, ids, {b: f"r{i % 2}" for i, b in enumerate(ids)})
    topic_of = np.array([("alpha", "beta", "gamma").index(k[0]) for k in fi.keys])
    sizes = np.array([12, 9, 7])
    res = balance_leaders_cluster_arrays(fi.rows, B, topic_of, np.maximum(0, sizes // B - 1), -(-sizes // B) + 1)
    assert f"peak_before={res.peak_before} peak_after={res.peak_after} leader_changes={res.n_changed} " in report[0]
    assert res.peak_after < res.peak_before and res.n_changed > 0
    plan = json.loads(outs[0][0])
    assert plan["version"] == 1 and len(plan["partitions"]) == res.n_changed   # changed rows only
    rows = {k: [ids[b] for b in r if b != NONE] for k, r in zip(fi.keys, fi.rows.tolist())}
    for e in plan["partitions"]:
        key = (e["topic"], e["partition"])
        assert e["replicas"] != rows[key] and sorted(e["replicas"]) == sorted(rows[key])
        rows[key] = e["replicas"]
    assert [rows[k] for k in fi.keys] == [[ids[b] for b in r if b != NONE] for r in res.rows.tolist()]
    # a cap nobody can meet: reported, exit status 1, an empty plan
    r = subprocess.run(progs[0] + base + ["--cluster-hi", "1", "--report"], capture_output=True, cwd=ROOT)
    assert r.returncode == 1 and b"status=INFEASIBLE_PROVEN" in r.stderr and json.loads(r.stdout)["partitions"] == []


def test_python_api_on_topics(kao):
    """balance_leaders_cluster on Topic objects of different RF: the per-topic assignments and the plan entries."""
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_cluster
    ids = np.array([5, 6, 7, 8])
    a = Topic(name="a", broker_ids=ids, rack_of=np.arange(4) % 2, n_racks=2, n_partitions=4, rf=3,
              current=np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [0, 1, 3]], dtype=np.uint16))
    b = Topic(name="b", broker_ids=ids, rack_of=np.arange(4) % 2, n_racks=2, n_partitions=3, rf=2, partition_ids=np.array([4, 8, 9]),
              current=np.array([[0, 1], [0, 2], [1, 0]], dtype=np.uint16))
    plan = balance_leaders_cluster([a, b], slack=0)
    res = plan.result
    rows = np.full((7, 3), NONE, dtype=np.int64)
    rows[:4], rows[4:, :2] = a.current, b.current
    assert (res.status, res.peak_after, res.n_changed) == ("OPTIMAL_PROVEN",) + cr.optimum(rows, [0, 0, 0, 0, 1, 1, 1], 4, 0, [1, 0], [1, 1])
    assert [x.shape for x in plan.assignments] == [(4, 3), (3, 2)]
    assert (np.concatenate([plan.assignments[0].ravel(), plan.assignments[1].ravel()]) == res.rows[res.rows != NONE]).all()
    assert len(plan.entries) == res.n_changed and all(set(r) <= set(ids.tolist()) for _, _, r in plan.entries)
    assert {(t, p) for t, p, _ in plan.entries} <= {("a", 0), ("a", 1), ("a", 2), ("a", 3), ("b", 4), ("b", 8), ("b", 9)}
    dry = balance_leaders_cluster([a, b], dry_run=True)
    assert dry.entries == [] and _numbers(dry.result) == _numbers(res)
