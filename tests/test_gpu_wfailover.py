"""kao_failover_order_weighted on the MI355X: the follower order that keeps the peak traffic a surviving broker leads after a broker
or rack failure low, by the synchronous rounds of section 4k run per failure scenario, with a lower bound per scenario (DESIGN.md
section 4l).  Every instance goes through `_checked`: the output rows equal the restatement of tests/wfailover_ref.py byte for byte,
the six values of every scenario and the counters equal it, the certificate recomputed from the returned rows is the reported one,
the status follows from the numbers, two calls give the same bytes and a dry run reports the same numbers on untouched rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import failover_ref as fr
import wfailover_ref as wf
from conftest import ROOT

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
COUNTERS = [0, 1, 2, 3, 5, 6, 7]


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def call(kao):
    from kafka_assignment_optimizer_amd.failover import failover_order_weighted_arrays
    return failover_order_weighted_arrays


def _same(a, b):
    return (a.rows.tobytes() == b.rows.tobytes() and a.scen.tobytes() == b.scen.tobytes() and a.n_reordered == b.n_reordered and
            a.status == b.status and a.stats.tolist() == b.stats.tolist())


def _checked(call, rows, B, rack_of, R, scope, weight, min_gain=0, max_rounds=0):
    """One instance through the GPU against the restatement.  Returns (result, restatement)."""
    rows = np.asarray(rows, dtype=np.int64)
    ref = wf.descend(rows, weight, B, rack_of, scope, R, min_gain, max_rounds)
    res = call(rows, B, rack_of, R, scope, weight, min_gain, max_rounds)
    again = call(rows, B, rack_of, R, scope, weight, min_gain, max_rounds)
    dry = call(rows, B, rack_of, R, scope, weight, min_gain, max_rounds, dry_run=True)
    scen = [[int(x) for x in s] for s in res.scen.tolist()]
    print(f"B={B} R={R} P={rows.shape[0]} W={rows.shape[1]} scope={scope} n_reordered={res.n_reordered} status={res.status} "
          f"stats={res.stats.tolist()} ref={ref['stats']}")
    assert res.rows.astype(np.int64).tobytes() == ref["rows"].tobytes()
    assert scen == ref["scen"], [g for g in range(len(scen)) if scen[g] != ref["scen"][g]][:10]
    assert res.stats[COUNTERS].tolist() == [ref["stats"][i] for i in COUNTERS]
    assert res.n_reordered == ref["n_reordered"] == sum(s[5] for s in scen)
    assert [s[4] for s in scen] == wf.lower_bound(res.rows, weight, B, rack_of, scope, R)
    assert all(s[4] <= s[3] <= s[2] for s in scen)
    assert res.status == ("OPTIMAL_PROVEN" if all(s[3] == s[4] for s in scen) else "FEASIBLE_BOUND_GAP")
    assert fr.check_rows(rows, res.rows, B, rack_of, scope) == res.n_reordered
    if ref["stats"][5] == 0:
        assert wf.stable(res.rows, weight, B, rack_of, scope, min_gain)
    assert _same(res, again)
    assert (dry.rows == rows).all() and dry.scen.tobytes() == res.scen.tobytes() and dry.n_reordered == res.n_reordered
    assert dry.status == res.status and dry.stats.tolist() == res.stats.tolist()
    return res, ref


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_matches_the_restatement(call):
    improved = proven = gaps = 0
    for i, (rows, B, rack_of, R) in enumerate(fr.small_family()):
        weight = wf.family_weights(i, len(rows))
        for scope in (0, 1):
            res, _ = _checked(call, rows, B, rack_of, R, scope, weight)
            assert int(res.scen[:, 0].max()) * rows.shape[1] <= 1024   # the 256-lane path
            improved += int((res.scen[:, 3] < res.scen[:, 2]).sum())
            proven += res.status == "OPTIMAL_PROVEN"
            gaps += res.status == "FEASIBLE_BOUND_GAP"
    print(f"improved scenarios: {improved}, calls proven: {proven}, with a gap: {gaps}")
    assert improved > 0 and proven > 0 and gaps > 0


# ---- 2. contention -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 4, 5])
def test_every_proposal_collides_at_the_first_elected_broker(call, B):
    """All leaders on broker 0, all of them electing broker 1: in broker scope scenario 0 holds every partition.  Equal weights: every
    key ties down to p.  Weights of 2^40 + a little: the loads pass 2^48.  1,500 partitions are 4,500 slots: the 1,024-lane path."""
    for P in (64, 257, 1500):
        for base in (0, 2 ** 40):
            rows, weight, B, rack_of, R = wf.contention_case(B, P, base)
            res, ref = _checked(call, rows, B, rack_of, R, 0, weight)
            assert res.stats[0] == 1 and int(res.scen[0, 0]) == P and res.n_reordered > 0
            assert res.stats[1] >= res.n_reordered // (B - 1)   # one source: few winners per round
            if base:
                assert int(res.scen[0, 2]) > 2 ** 40 * P >= 2 ** 46 and (P < 257 or int(res.scen[0, 2]) > 2 ** 48)
    rows, weight, B, rack_of, R = wf.contention_case(B, 257)
    none, _ = _checked(call, rows, B, rack_of, R, 0, weight, min_gain=257 * 5)   # no gap is that large
    assert none.n_reordered == 0 and none.stats[0] == 1 and none.stats[1] == 0 and none.stats[5] == 0
    one, _ = _checked(call, rows, B, rack_of, R, 0, weight, max_rounds=1)
    assert one.stats[1] == 1 and one.stats[5] == 1 and one.stats[7] == 1


# ---- 3. the mid instance -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    rows, B, rack_of, R = fr.many_instance()
    return rows, B, rack_of, R, wf.lognormal_weights(len(rows), 0.7, 5)


def test_mid_instance_in_rack_scope(call, mid):
    """300 brokers in 10 racks, 9,000 partitions at RF 3: 900 partitions = 2,700 slots per workgroup, 1,024 lanes."""
    rows, B, rack_of, R, weight = mid
    res, _ = _checked(call, rows, B, rack_of, R, 1, weight)
    assert res.stats[0] == 10 and int(res.scen[:, 0].max()) == 900
    assert res.stats[7] > 10 and int(res.scen[:, 3].max()) < int(res.scen[:, 2].max())


def test_mid_instance_in_broker_scope(call, mid):
    """300 workgroups of 256 lanes, more than the compute units."""
    rows, B, rack_of, R, weight = mid
    res, _ = _checked(call, rows, B, rack_of, R, 0, weight)
    assert res.stats[0] == 300 and int(res.scen[:, 0].max()) * 3 <= 1024
    assert int(res.scen[:, 3].max()) < int(res.scen[:, 2].max())


# ---- 4. unit weights against the exact kernel of section 4i --------------------------------------------------------------------------
def test_unit_weights_bracket_the_exact_kernel(call):
    from kafka_assignment_optimizer_amd.failover import failover_order_arrays
    for rows, B, rack_of, R in fr.small_family()[:20]:
        for scope in (0, 1):
            res, _ = _checked(call, rows, B, rack_of, R, scope, np.ones(len(rows), dtype=np.int64))
            exact = failover_order_arrays(rows, B, rack_of, R, scope).scen
            assert (res.scen[:, 2] == exact[:, 2]).all() and (res.scen[:, :2] == exact[:, :2]).all()
            assert (res.scen[:, 4] <= exact[:, 3]).all() and (exact[:, 3] <= res.scen[:, 3]).all()


# ---- 5. limits and edges -------------------------------------------------------------------------------------------------------------
def test_broker_limit(call):
    """KAO_FAILOVER_MAX_BROKERS brokers: 128,000 bytes of LDS per workgroup, broker index 7,999 in use."""
    rows, B, rack_of, R = fr.limit_instance(8000)
    assert B == 8000 and (rows[:, 0] == B - 1).any()
    res, _ = _checked(call, rows, B, rack_of, R, 0, wf.lognormal_weights(len(rows), 0.7, 8))
    assert res.stats[0] == 40 and res.n_reordered > 0 and int(res.scen[B - 1, 0]) > 0


CHILD = """
import pickle, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import failover_ref as fr
import wfailover_ref as wf
import kafka_assignment_optimizer_amd as k
from kafka_assignment_optimizer_amd.failover import failover_order_weighted_arrays as call
k.init(0)
rows, B, rack_of, R = fr.limit_instance({B})
weight = wf.lognormal_weights(len(rows), 0.7, 8)
out = [call(rows, B, rack_of, R, 0, weight, 0, 0, dry_run=dry) for dry in (False, False, True)]   # the calls of _checked, in its order
pickle.dump(out, open({out!r}, "wb"))
"""


@pytest.mark.parametrize("B", [2048, 2049])
def test_dynamic_lds_opt_in_edge_in_a_fresh_process(kao, tmp_path, B):
    """16 B bytes of dynamic LDS: exactly 32 KiB at B = 2048, which the entry point launches without opening the kernel, and 16
    bytes more at B = 2049, which it opens the kernel for.  The opt-in is remembered per process, so the three calls of `_checked`
    run in a fresh child process, the first of them the first launch of k_wfo_solve there; the parent compares what the child got."""
    import pickle
    assert fr.weighted_lds_bytes(B) == {2048: 32768, 2049: 32784}[B]
    out = str(tmp_path / "result.pkl")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), B=B, out=out)
    r = subprocess.run([sys.executable, "-c", code], timeout=120, capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = iter(pickle.load(open(out, "rb")))
    dry_flags = iter((False, False, True))

    def replay(rows, B, rack_of, R, scope, weight, min_gain=0, max_rounds=0, dry_run=False):
        assert dry_run == next(dry_flags)
        return next(got)

    rows, B, rack_of, R = fr.limit_instance(B)
    res, _ = _checked(replay, rows, B, rack_of, R, 0, wf.lognormal_weights(len(rows), 0.7, 8))
    assert res.stats[0] == 40 and res.n_reordered > 0 and int(res.scen[B - 1, 0]) > 0


def test_edge_cases(call):
    res = call(np.zeros((0, 3)), 4, [0, 1, 0, 1], 2, 0, np.zeros(0, dtype=np.int64))   # no partition
    assert res.scen.tolist() == [[0] * 6] * 4 and res.status == "OPTIMAL_PROVEN" and res.n_reordered == 0
    assert res.stats[COUNTERS].tolist() == [0, 0, 0, 0, 0, 4, 0]
    rows, B, rack_of, R = fr.small_family()[5]
    weight = wf.family_weights(5, len(rows))
    assert (rows == NONE).any() and not (rows[:, 1:] == NONE).all()   # mixed padding
    for scope in (0, 1):
        res, _ = _checked(call, rows, B, rack_of, R, scope, np.zeros(len(rows), dtype=np.int64))   # nothing weighs anything
        assert res.n_reordered == 0 and not res.scen[:, 2:5].any() and res.status == "OPTIMAL_PROVEN" and res.stats[1] == 0
        res, _ = _checked(call, rows[:, :1], B, rack_of, R, scope, weight)   # width 1: everything is offline
        assert not res.scen[:, 0].any() and int(res.scen[:, 1].sum()) == len(rows) and res.status == "OPTIMAL_PROVEN"
        res, _ = _checked(call, rows, B, rack_of, R, scope, weight, min_gain=2 ** 64 - 1)
        assert res.n_reordered == 0
    res, _ = _checked(call, np.zeros((5, 1)), 1, [0], 1, 0, [3, 0, 4, 1, 9])   # one broker: no survivor
    assert res.scen.tolist() == [[0, 5, 0, 0, 0, 0]]
    rng = np.random.default_rng(1)
    rows = np.array([rng.permutation(6)[:3] for _ in range(20)])
    res, _ = _checked(call, rows, 6, np.zeros(6, dtype=np.int64), 1, 1, np.arange(20) + 1)   # one rack in rack scope
    assert res.scen.tolist() == [[0, 20, 0, 0, 0, 0]]
    # a partition of weight 0 never moves, whatever the loads around it
    rows, weight, B, rack_of, R = wf.contention_case(4, 64)
    weight[::3] = 0
    res, _ = _checked(call, rows, B, rack_of, R, 0, weight)
    assert res.n_reordered > 0 and (res.rows[::3] == rows[::3]).all()


def test_invalid_arguments_leave_the_rows_alone(kao):
    """Every invalid argument of include/kao.h gives KAO_ERR_INVALID on a machine with a device too."""
    import test_wfailover_ref as host
    for what, change in host.INVALID:
        kw = dict(rows=host.ROWS)
        kw.update(change)
        assert host._call(**kw) == -1, what   # (_call asserts that the row buffer is unchanged)


# ---- 6. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-failover")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.failover"])


def _both(args, tmp_path, tag):
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"{tag}{i}.json"
        r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    return json.loads(outs[0][0]), outs[0][1].splitlines()


def test_cli_on_the_readme_example(kao, tmp_path):
    """The README topic with tests/golden/readme_traffic.json in both scopes: both tools print the same plan and the same report,
    and the report is the library's."""
    from kafka_assignment_optimizer_amd import failover as fo
    from kafka_assignment_optimizer_amd.leaders import parse_traffic
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    golden = os.path.join(ROOT, "tests", "golden")
    ids = list(range(20))
    racks = {int(k): v for k, v in json.load(open(os.path.join(golden, "readme_racks.json"))).items()}
    base = ["--current", os.path.join(golden, "readme_current.json"), "--broker-list", ",".join(str(b) for b in ids), "--racks",
            os.path.join(golden, "readme_racks.json")]
    doc = json.load(open(os.path.join(golden, "readme_current.json")))
    table = parse_traffic(json.load(open(os.path.join(golden, "readme_traffic.json"))))
    for scope in ("broker", "rack"):
        plan, report = _both(base + ["--scope", scope, "--traffic", os.path.join(golden, "readme_traffic.json")], tmp_path, "readme" + scope)
        lib = fo.failover_order_weighted(doc, scope, table, broker_list=ids, racks=racks)
        assert report == fo.weighted_report_lines(lib) and report[-1].startswith(f"weighted: scope={scope} scenarios=")
        assert [(e["topic"], e["partition"], e["replicas"]) for e in plan["partitions"]] == lib.entries


def test_cli_weighted_end_to_end(kao, tmp_path):
    """cli/kao-failover --traffic / --sizes and the Python twin on a three-topic document of mixed RF: the same bytes, a plan of the
    changed rows only, which applied to the document gives the library's rows; the report carries the library's numbers; without
    the new flags both tools give what kao_failover_order gives."""
    from kafka_assignment_optimizer_amd import failover as fo
    from kafka_assignment_optimizer_amd.leaders import parse_traffic, plan_text, weights_for
    from kafka_assignment_optimizer_amd.waves import parse_sizes
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(7)
    B, ids = 8, [100 + 3 * i for i in range(8)]
    doc, traffic, logdirs = {"version": 1, "partitions": []}, {"version": 1, "partitions": []}, {}
    for name, P, rf in (("alpha", 24, 3), ("be-ta", 9, 2), ("gamma", 7, 1), ("delta", 16, 4)):
        for p in range(P):
            r = rng.permutation(B)[:rf]
            if rng.random() < 0.7 and (r[:2] < 2).any():   # brokers 0 and 1 lead or are elected first where they can
                j = int(np.nonzero(r[:2] < 2)[0][0])
                r[[min(1, rf - 1), j]] = r[[j, min(1, rf - 1)]]
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
            w = int(rng.integers(1, 1000))
            if not (name == "gamma" and p == 6):   # one partition is left to --default-weight
                traffic["partitions"].append({"topic": name, "partition": p, "weight": w})
                for b in r:
                    logdirs.setdefault(ids[b], []).append({"partition": f"{name}-{p}", "size": w * 1024 - int(b), "offsetLag": 0, "isFuture": False})
    racks = {b: f"r{i % 3}" for i, b in enumerate(ids)}
    cur_path, racks_path, traffic_path, sizes_path = (tmp_path / n for n in ("current.json", "racks.json", "traffic.json", "logdirs.txt"))
    cur_path.write_text(json.dumps(doc))
    racks_path.write_text(json.dumps({str(b): r for b, r in racks.items()}))
    traffic_path.write_text(json.dumps(traffic))
    sizes_path.write_text("Querying brokers for log directories information\n" + json.dumps(
        {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": "/d", "error": None, "partitions": e}]} for b, e in sorted(logdirs.items())]}) + "\n")
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path)]
    fi = fo.parse_current(doc, ids, racks)
    moved = 0
    for scope in ("broker", "rack"):
        for tag, flags, table in (("traffic", ["--traffic", str(traffic_path)], parse_traffic(traffic)),
                                  ("sizes", ["--sizes", str(sizes_path)], parse_sizes(sizes_path.read_text()))):
            for prog in PROGS:   # gamma-6 has no weight
                r = subprocess.run(prog + base + ["--scope", scope] + flags, capture_output=True, cwd=ROOT)
                assert r.returncode == 1 and b"gamma-6" in r.stderr, (prog, r.stderr)
            plan, report = _both(base + ["--scope", scope] + flags + ["--default-weight", "77", "--min-gain", "3"], tmp_path, tag + scope)
            weight = weights_for(fi.keys, table, 77)
            assert weight[fi.keys.index(("gamma", 6))] == 77 and (weight > 0).all()
            lib = fo.plan_input_weighted(fi, scope, weight, min_gain=3)
            res = lib.result
            assert report == fo.weighted_report_lines(lib)
            assert report[-1] == (f"weighted: scope={scope} scenarios={len(res.scen)} worst_peak_before={int(res.scen[:, 2].max())} "
                                  f"worst_peak_after={int(res.scen[:, 3].max())} worst_lower_bound={int(res.scen[:, 4].max())} proven={res.stats[6]} "
                                  f"offline={int(res.scen[:, 1].sum())} reordered={res.n_reordered} rounds={res.stats[1]} moves={res.stats[2]} "
                                  f"launches={res.stats[4]}")
            assert all(line.startswith("scenario=") and " lower_bound=" in line for line in report[:-1]) and len(report) > 1
            assert plan["version"] == 1 and len(plan["partitions"]) == res.n_reordered   # changed rows only
            rows = {k: [ids[b] for b in r if b != NONE] for k, r in zip(fi.keys, fi.rows.tolist())}
            for e in plan["partitions"]:
                key = (e["topic"], e["partition"])
                assert e["replicas"] != rows[key] and sorted(e["replicas"]) == sorted(rows[key]) and e["replicas"][0] == rows[key][0]
                rows[key] = e["replicas"]
            assert [rows[k] for k in fi.keys] == [[ids[b] for b in r if b != NONE] for r in res.rows.tolist()]
            moved += res.n_reordered
            one, report1 = _both(base + ["--scope", scope] + flags + ["--default-weight", "77", "--max-rounds", "1"], tmp_path, tag + scope + "one")
            assert 0 < int(report1[-1].split(" rounds=")[1].split()[0]) <= res.stats[0]   # at most one round per scenario
            dry, report2 = _both(base + ["--scope", scope] + flags + ["--default-weight", "77", "--min-gain", "3", "--dry-run"], tmp_path, tag + scope + "dry")
            assert dry["partitions"] == [] and report2 == report
        plain, report = _both(base + ["--scope", scope], tmp_path, "plain" + scope)   # without the new flags: kao_failover_order
        exact = fo.plan_input(fi, scope)
        assert report == fo.report_lines(exact) and json.dumps(plain) == json.dumps(json.loads(plan_text(exact.entries)))
        assert (tmp_path / f"plain{scope}0.json").read_text() == plan_text(exact.entries)
    assert moved > 0
    for prog in PROGS:   # usage errors exit with 2 on a machine with a device too
        assert subprocess.run(prog + base + ["--scope", "rack", "--traffic", str(traffic_path), "--sizes", str(sizes_path)], capture_output=True, cwd=ROOT).returncode == 2
        assert subprocess.run(prog + base + ["--scope", "rack", "--min-gain", "3"], capture_output=True, cwd=ROOT).returncode == 2


def test_python_api_on_topics(kao):
    """failover_order_weighted on Topic objects of different RF: the per-topic assignments and the plan entries."""
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.failover import failover_order_weighted
    ids = np.array([5, 6, 7, 8])
    rack_of = np.arange(4) % 2
    a = Topic(name="a", broker_ids=ids, rack_of=rack_of, n_racks=2, n_partitions=4, rf=3,
              current=np.array([[0, 1, 2], [0, 1, 3], [0, 1, 2], [0, 1, 3]], dtype=np.uint16))
    b = Topic(name="b", broker_ids=ids, rack_of=rack_of, n_racks=2, n_partitions=3, rf=2, partition_ids=np.array([4, 8, 9]),
              current=np.array([[0, 1], [0, 2], [1, 0]], dtype=np.uint16))
    table = {("a", 0): 40, ("a", 1): 30, ("a", 2): 20, ("a", 3): 10, ("b", 4): 25, ("b", 8): 15}
    plan = failover_order_weighted([a, b], "broker", table, default_weight=5)
    res = plan.result
    rows = np.full((7, 3), NONE, dtype=np.int64)
    rows[:4], rows[4:, :2] = a.current, b.current
    ref = wf.descend(rows, [40, 30, 20, 10, 25, 15, 5], 4, rack_of, 0, 2)
    assert plan.weight.tolist() == [40, 30, 20, 10, 25, 15, 5]
    assert res.rows.astype(np.int64).tolist() == ref["rows"].tolist() and res.scen.tolist() == ref["scen"]
    assert int(res.scen[0, 3]) < int(res.scen[0, 2]) == 5 + 100 + 25
    assert [x.shape for x in plan.assignments] == [(4, 3), (3, 2)] and (plan.assignments[1] == b.current).all()
    assert len(plan.entries) == res.n_reordered > 0 and all(t == "a" and r[0] == 5 for t, _, r in plan.entries)
    same = failover_order_weighted([a, b], 0, [[40, 30, 20, 10], [25, 15, 5]])
    assert same.result.rows.tobytes() == res.rows.tobytes()
    dry = failover_order_weighted([a, b], "broker", table, default_weight=5, dry_run=True)
    assert dry.entries == [] and dry.result.scen.tobytes() == res.scen.tobytes()
