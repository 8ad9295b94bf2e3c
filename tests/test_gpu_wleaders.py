"""kao_balance_leaders_weighted on the MI355X: the preferred leaders of all topics chosen so that the traffic a broker leads has a
low peak, by synchronous rounds of a deterministic descent, with a lower bound that proves the peak optimal where the two meet
(DESIGN.md section 4k).  Every instance is held byte for byte against the restatement of the rounds in tests/wleaders_ref.py, on the
single-workgroup path and on the multi-launch path; every result is checked for the invariants: rows are one swap with slot 0 away
from their input, no move is left, the bound recomputed from the returned rows is the reported one, two calls give the same bytes,
dry_run reports the same numbers."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wleaders_ref as wr
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
ONE, MULTI = 1, 2


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def call(kao):
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_weighted_arrays
    return balance_leaders_weighted_arrays


@contextlib.contextmanager
def forced(path):
    """The kernel path of this thread's calls (kao_wleaders_test_path), put back on the way out."""
    from kafka_assignment_optimizer_amd import _ffi
    was = _ffi.load().kao_wleaders_test_path(path)
    assert was >= 0
    try:
        yield
    finally:
        _ffi.load().kao_wleaders_test_path(was)


def _numbers(res):
    return res.status, res.n_changed, res.peak_before, res.peak_after, res.lower_bound


def _checked(call, rows, weight, B, min_gain=0, max_rounds=0, path=None):
    """One instance through the GPU against the restatement: bytes, numbers, stats[0..2]; twice, and once with dry_run; every
    invariant.  Returns (result, restatement)."""
    rows = np.asarray(rows, dtype=np.int64)
    ref = wr.descend(rows, weight, B, min_gain, max_rounds)
    with forced(0 if path is None else path):
        res = call(rows, B, weight, min_gain, max_rounds)
        again = call(rows, B, weight, min_gain, max_rounds)
        dry = call(rows, B, weight, min_gain, max_rounds, dry_run=True)
    print(f"B={B} P={len(rows)} gpu={_numbers(res)} stats={res.stats.tolist()} ref rounds={ref['rounds']} moves={ref['moves']} proposals={ref['proposals']}")
    assert res.rows.astype(np.int64).tobytes() == ref["rows"].tobytes()
    assert (res.n_changed, res.peak_before, res.peak_after) == (ref["n_changed"], ref["peak_before"], ref["peak_after"])
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[5] == int(ref["more"]) and res.stats[7] == ref["leading"]
    assert (res.lower_bound, int(res.stats[6])) == wr.lower_bound(res.rows, weight, B)
    assert res.lower_bound <= res.peak_after <= res.peak_before
    assert res.status == ("OPTIMAL_PROVEN" if res.peak_after == res.lower_bound else "FEASIBLE_BOUND_GAP")
    if not ref["more"]:
        assert wr.stable(rows, res.rows, weight, B, min_gain)
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()
    if path is not None:
        assert res.stats[4] == (1 if path == ONE else 0)
    return res, ref


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_matches_the_restatement(call):
    proven = 0
    for seed in range(120):
        rows, weight, B = wr.small_case(seed)
        res, _ = _checked(call, rows, weight, B)
        assert res.stats[4] == 1, seed   # small inputs run in one workgroup
        proven += res.status == "OPTIMAL_PROVEN"
    print(f"proven optimal: {proven} of 120")


# ---- 2. contention -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [ONE, MULTI])
@pytest.mark.parametrize("B", [2, 3, 4])
def test_every_proposal_collides_at_one_source(call, B, path):
    """All leaders on broker 0.  Equal weights: every key ties down to p.  Weights of 2^40 + a little: the loads pass 2^32 and 2^48."""
    for P in (64, 257, 1500):
        for base in (0, 2 ** 40):
            rows, weight = wr.collide_case(B, P, base)
            res, ref = _checked(call, rows, weight, B, path=path)
            assert res.n_changed > 0 and res.stats[0] >= res.n_changed // (B - 1)   # one source: few winners per round
            if base:
                assert res.peak_before > 2 ** 40 * P >= 2 ** 46 and (P < 257 or res.peak_before > 2 ** 48)
    rows, weight = wr.collide_case(B, 257)
    none, _ = _checked(call, rows, weight, B, min_gain=257 * 5, path=path)   # no gap is that large
    assert none.n_changed == 0 and none.stats[0] == 0 and none.stats[5] == 0
    one, ref = _checked(call, rows, weight, B, max_rounds=1, path=path)
    assert one.stats[0] == 1 and one.stats[5] == 1 and ref["more"]


# ---- 3. the mid instance: the multi-launch path by size -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    return wr.lognormal_case(300, 6000, 3, 0.7, 5)


def test_mid_instance_runs_the_multi_launch_path(call, mid):
    rows, weight = mid
    res, ref = _checked(call, rows, weight, 300)
    assert res.stats[4] == 0 and res.stats[3] > 1
    assert res.peak_after < res.peak_before and ref["rounds"] > 50


# ---- 4. one input down both paths ----------------------------------------------------------------------------------------------------
def test_both_paths_give_the_same_bytes(call, mid):
    rows, weight = mid
    with forced(ONE):
        a = call(rows, 300, weight)
    with forced(MULTI):
        b = call(rows, 300, weight)
    assert a.stats[4] == 1 and b.stats[4] == 0
    assert a.rows.tobytes() == b.rows.tobytes() and _numbers(a) == _numbers(b)
    assert a.stats[[0, 1, 2, 5, 6, 7]].tolist() == b.stats[[0, 1, 2, 5, 6, 7]].tolist()
    for seed in (1, 2, 5):   # and on small inputs, limits included
        rows, weight, B = wr.small_case(seed)
        for kw in (dict(), dict(max_rounds=2), dict(min_gain=9)):
            _checked(call, rows, weight, B, path=ONE, **kw)
            _checked(call, rows, weight, B, path=MULTI, **kw)


# ---- 4b. the rounds against the batches of the multi-launch path (32 rounds between two reads of the counts) -------------------------
@pytest.mark.parametrize("path", [ONE, MULTI])
def test_last_round_with_a_proposal_is_the_last_of_a_batch(call, path):
    """The descent takes exactly 32 rounds (tests/test_wleaders_ref.py holds the generator to it): the first batch is full and the
    first round of the second is empty.  Launches: init and the peak before, two batches of 32 rounds of two, rank, finish, scan."""
    rows, weight = wr.lognormal_case(6, 200, 3, 0.7, 26)
    res, _ = _checked(call, rows, weight, 6, path=path)
    assert res.stats[0] == 32 and res.stats[5] == 0
    if path == MULTI:
        assert res.stats[3] == 2 + 2 * 64 + 3


@pytest.mark.parametrize("path", [ONE, MULTI])
def test_max_rounds_at_and_around_a_batch(call, path):
    """Launches on the multi-launch path: the 5 around the rounds, 2 a round enqueued (a batch is cut at max_rounds) and, when every
    one of max_rounds rounds had a proposal, the probe of 1.  At 64 the second batch holds the first empty round: no probe."""
    rows, weight = wr.lognormal_case(6, 300, 3, 0.7, 7)
    for limit, rounds, more, launches in ((31, 31, 1, 5 + 2 * 31 + 1), (32, 32, 1, 5 + 2 * 32 + 1), (33, 33, 1, 5 + 2 * 33 + 1), (64, 52, 0, 5 + 2 * 64)):
        res, _ = _checked(call, rows, weight, 6, max_rounds=limit, path=path)
        assert (res.stats[0], res.stats[5]) == (rounds, more), limit
        if path == MULTI:
            assert res.stats[3] == launches, limit


# ---- 5. unit weights against the exact solver of section 4j --------------------------------------------------------------------------
def test_unit_weights_bracket_the_exact_cluster_balance(call):
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_cluster_arrays
    for seed in range(20):
        rows, _, B = wr.small_case(seed)
        P = len(rows)
        res, _ = _checked(call, rows, np.ones(P, dtype=np.int64), B)
        exact = balance_leaders_cluster_arrays(rows, B, np.zeros(P, dtype=np.int32), [0], [P])
        assert exact.status == "OPTIMAL_PROVEN"
        assert res.lower_bound <= exact.peak_after <= res.peak_after, (seed, res.lower_bound, exact.peak_after, res.peak_after)


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------
def test_edge_cases(call):
    res = call(np.zeros((0, 3)), 4, np.zeros(0, dtype=np.int64))   # no partition
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0) and res.stats[[0, 1, 2, 5, 6, 7]].tolist() == [0] * 6
    rows, weight, B = wr.small_case(3)
    for path in (ONE, MULTI):
        res, _ = _checked(call, rows, np.zeros(len(rows), dtype=np.int64), B, path=path)   # nothing weighs anything
        assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0) and res.stats[0] == 0
        res, _ = _checked(call, rows[:, :1], weight, B, path=path)   # width 1: every load is forced
        assert res.status == "OPTIMAL_PROVEN" and res.n_changed == 0 and res.peak_after == res.peak_before == res.lower_bound
        res, _ = _checked(call, np.zeros((5, 1)), [3, 0, 4, 1, 9], 1, path=path)   # one broker
        assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 17, 17, 17) and res.stats[7] == 1
        r = np.array([[65533, 0, 7], [65533, 65532, NONE], [65533, 9, 65532], [65533, NONE, NONE]])
        res, _ = _checked(call, r, [10, 20, 30, 5], 65534, path=MULTI if path == MULTI else None)   # (the single workgroup holds 2,048 brokers)
        assert res.stats[4] == 0 and res.n_changed == 3 and res.peak_after == 30 and res.status == "OPTIMAL_PROVEN"
    with forced(ONE), pytest.raises(Exception) as e:   # the hook does not bend the LDS limit
        call(r, 65534, [10, 20, 30, 5])
    assert e.value.code == -2


def test_invalid_arguments_leave_the_rows_alone(kao):
    """Every invalid argument of include/kao.h gives KAO_ERR_INVALID on a machine with a device too."""
    import test_wleaders_ref as host
    for what, change in host.INVALID:
        kw = dict(rows=[[0, 1], [2, 3], [1, 2]], B=4, weight=[5, 6, 7])
        kw.update(change)
        assert host._call(**kw) == -1, what   # (_call asserts that the row buffer is unchanged)


# ---- 7. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"])


def _both(args, tmp_path, tag):
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"{tag}{i}.json"
        r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    report = outs[0][1].splitlines()
    assert len(report) == 1 and report[0].startswith("weighted: status=")
    return json.loads(outs[0][0]), report[0]


def test_cli_on_the_readme_example(kao, tmp_path):
    """The README topic with hand-written weights (tests/golden/readme_traffic.json) and with its log-dir sizes: no broker leads two
    partitions, so nothing moves and the heaviest partition is the proven peak; both tools say so in the same bytes."""
    from kafka_assignment_optimizer_amd.waves import parse_sizes
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    golden = os.path.join(ROOT, "tests", "golden")
    base = ["--current", os.path.join(golden, "readme_current.json"), "--broker-list", ",".join(str(b) for b in range(20)), "--racks",
            os.path.join(golden, "readme_racks.json")]
    plan, report = _both(base + ["--traffic", os.path.join(golden, "readme_traffic.json")], tmp_path, "traffic")
    assert plan == {"version": 1, "partitions": []}
    assert report == "weighted: status=OPTIMAL_PROVEN peak_before=950 peak_after=950 lower_bound=950 leader_changes=0 rounds=0 moves=0 launches=6"
    plan, report = _both(base + ["--sizes", os.path.join(golden, "readme_log_dirs.txt")], tmp_path, "sizes")
    sizes = parse_sizes(open(os.path.join(golden, "readme_log_dirs.txt")).read())
    assert plan["partitions"] == [] and f"peak_before={max(sizes.values())} peak_after={max(sizes.values())} " in report
    assert max(sizes.values()) == 1048576000


def test_cli_weighted_end_to_end(kao, tmp_path):
    """cli/kao-leaders --traffic / --sizes and the Python twin on a three-topic document of mixed RF: the same bytes, a plan of the
    changed rows only, which applied to the document gives the library's rows; --sizes weighs as waves.parse_sizes reads the file."""
    from kafka_assignment_optimizer_amd.failover import parse_current
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_weighted_arrays, parse_traffic, weights_for
    from kafka_assignment_optimizer_amd.waves import parse_sizes
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(7)
    B, ids = 8, [100 + 3 * i for i in range(8)]
    doc, traffic, logdirs = {"version": 1, "partitions": []}, {"version": 1, "partitions": []}, {}
    for name, P, rf in (("alpha", 12, 3), ("be-ta", 9, 2), ("gamma", 7, 1)):
        for p in range(P):
            r = rng.permutation(B)[:rf]
            if rng.random() < 0.7 and (r < 2).any():   # brokers 0 and 1 lead what they hold
                j = int(np.nonzero(r < 2)[0][0])
                r[[0, j]] = r[[j, 0]]
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
            w = int(rng.integers(1, 1000))
            if not (name == "gamma" and p == 6):   # one partition is left to --default-weight
                traffic["partitions"].append({"topic": name, "partition": p, "weight": w})
                for b in r:
                    logdirs.setdefault(ids[b], []).append({"partition": f"{name}-{p}", "size": w * 1024 - int(b), "offsetLag": 0, "isFuture": False})
    cur_path, racks_path, traffic_path, sizes_path = (tmp_path / n for n in ("current.json", "racks.json", "traffic.json", "logdirs.txt"))
    cur_path.write_text(json.dumps(doc))
    racks_path.write_text(json.dumps({str(b): f"r{i % 2}" for i, b in enumerate(ids)}))
    traffic_path.write_text(json.dumps(traffic))
    sizes_path.write_text("Querying brokers for log directories information\n" + json.dumps(
        {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": "/d", "error": None, "partitions": e}]} for b, e in sorted(logdirs.items())]}) + "\n")
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path)]
    fi = parse_current(doc, ids, {b: f"r{i % 2}" for i, b in enumerate(ids)})
    for tag, flags, table in (("traffic", ["--traffic", str(traffic_path)], parse_traffic(traffic)),
                              ("sizes", ["--sizes", str(sizes_path)], parse_sizes(sizes_path.read_text()))):
        for prog in PROGS:   # gamma-6 has no weight
            r = subprocess.run(prog + base + flags, capture_output=True, cwd=ROOT)
            assert r.returncode == 1 and b"gamma-6" in r.stderr, (prog, r.stderr)
        plan, report = _both(base + flags + ["--default-weight", "77", "--min-gain", "3"], tmp_path, tag)
        weight = weights_for(fi.keys, table, 77)
        assert weight[fi.keys.index(("gamma", 6))] == 77 and (weight > 0).all()
        res = balance_leaders_weighted_arrays(fi.rows, B, weight, min_gain=3)
        assert report == (f"weighted: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} lower_bound={res.lower_bound} "
                          f"leader_changes={res.n_changed} rounds={res.stats[0]} moves={res.stats[1]} launches={res.stats[3]}")
        assert res.peak_after < res.peak_before and res.n_changed > 0
        assert plan["version"] == 1 and len(plan["partitions"]) == res.n_changed   # changed rows only
        rows = {k: [ids[b] for b in r if b != NONE] for k, r in zip(fi.keys, fi.rows.tolist())}
        for e in plan["partitions"]:
            key = (e["topic"], e["partition"])
            assert e["replicas"] != rows[key] and sorted(e["replicas"]) == sorted(rows[key])
            rows[key] = e["replicas"]
        assert [rows[k] for k in fi.keys] == [[ids[b] for b in r if b != NONE] for r in res.rows.tolist()]
        one, report1 = _both(base + flags + ["--default-weight", "77", "--max-rounds", "1"], tmp_path, tag + "one")
        assert " rounds=1 " in report1 and 0 < len(one["partitions"]) <= res.n_changed
    for prog in PROGS:   # usage errors exit with 2 on a machine with a device too
        assert subprocess.run(prog + base + ["--traffic", str(traffic_path), "--cluster"], capture_output=True, cwd=ROOT).returncode == 2
        assert subprocess.run(prog + base + ["--traffic", str(traffic_path), "--sizes", str(sizes_path)], capture_output=True, cwd=ROOT).returncode == 2
        assert subprocess.run(prog + base + ["--min-gain", "3"], capture_output=True, cwd=ROOT).returncode == 2


def test_python_api_on_topics(kao):
    """balance_leaders_weighted on Topic objects of different RF: the per-topic assignments and the plan entries."""
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_weighted
    ids = np.array([5, 6, 7, 8])
    a = Topic(name="a", broker_ids=ids, rack_of=np.arange(4) % 2, n_racks=2, n_partitions=4, rf=3,
              current=np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [0, 1, 3]], dtype=np.uint16))
    b = Topic(name="b", broker_ids=ids, rack_of=np.arange(4) % 2, n_racks=2, n_partitions=3, rf=2, partition_ids=np.array([4, 8, 9]),
              current=np.array([[0, 1], [0, 2], [1, 0]], dtype=np.uint16))
    table = {("a", 0): 40, ("a", 1): 30, ("a", 2): 20, ("a", 3): 10, ("b", 4): 25, ("b", 8): 15}
    plan = balance_leaders_weighted([a, b], table, default_weight=5)
    res = plan.result
    rows = np.full((7, 3), NONE, dtype=np.int64)
    rows[:4], rows[4:, :2] = a.current, b.current
    ref = wr.descend(rows, [40, 30, 20, 10, 25, 15, 5], 4)
    assert plan.weight.tolist() == [40, 30, 20, 10, 25, 15, 5]
    assert res.rows.astype(np.int64).tolist() == ref["rows"].tolist() and res.peak_after == ref["peak_after"] < res.peak_before == 140
    assert [x.shape for x in plan.assignments] == [(4, 3), (3, 2)]
    assert (np.concatenate([plan.assignments[0].ravel(), plan.assignments[1].ravel()]) == res.rows[res.rows != NONE]).all()
    assert len(plan.entries) == res.n_changed > 0 and all(set(r) <= set(ids.tolist()) for _, _, r in plan.entries)
    assert {(t, p) for t, p, _ in plan.entries} <= {("a", 0), ("a", 1), ("a", 2), ("a", 3), ("b", 4), ("b", 8), ("b", 9)}
    same = balance_leaders_weighted([a, b], [[40, 30, 20, 10], [25, 15, 5]])
    assert same.result.rows.tobytes() == res.rows.tobytes()
    dry = balance_leaders_weighted([a, b], table, default_weight=5, dry_run=True)
    assert dry.entries == [] and _numbers(dry.result) == _numbers(res)
