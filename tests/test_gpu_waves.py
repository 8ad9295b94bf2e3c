"""kao_plan_waves on the MI355X: a plan split into waves with at most k partition movements per broker per wave.  Every result
is checked by an independent restatement (tests/waves_ref.py): coverage, caps, metadata-only partitions in wave 0, the lower
bound, and at most as many waves as the sequential first fit in degree-descending order; small instances also against the
exact optimum (HiGHS) and bit for bit against the host restatement of the kernel's best-of-orders first fit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import waves_ref as wr
from conftest import GOLDEN, ROOT, load_golden

pytestmark = pytest.mark.gpu
NONE = 0xFFFF


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _run(cur, tgt, B, k, seed=1):
    from kafka_assignment_optimizer_amd.waves import plan_waves_arrays
    return plan_waves_arrays(cur, tgt, B, k, seed)


def _valid(cur, tgt, B, k, seed=1):
    wave, nw, lb = _run(cur, tgt, B, k, seed)
    wr.check(cur, tgt, k, wave, nw, lb)
    assert nw <= wr.first_fit_waves(cur, tgt, k)
    return wave, nw, lb


def test_kat_readme_optimal_plan(kao):
    """The README's optimal plan moves only partition 1 ([8,19] -> [8,1], README.md:88): one wave holding it, proven optimal."""
    from kafka_assignment_optimizer_amd.waves import plan_waves
    plan = {"version": 1, "partitions": [{"topic": "x.y.z.t", "partition": 1, "replicas": [8, 1]}]}
    for k in (1, 2):
        res = plan_waves(load_golden("readme_current.json"), plan, k)
        assert (res.n_waves, res.lower_bound, res.optimal) == (1, 1, True)
        assert res.wave.tolist() == [-1, 0] + [-1] * 8
        assert res.waves == [{"version": 1, "partitions": [{"topic": "x.y.z.t", "partition": 1, "replicas": [8, 1]}]}]


@pytest.mark.parametrize("k", [1, 2, 3])
def test_readme_proposal_matches_the_ilp_optimum(kao, k):
    from kafka_assignment_optimizer_amd.waves import parse_pair, plan_waves
    cur, prop = load_golden("readme_current.json"), load_golden("readme_proposal.json")
    res = plan_waves(cur, prop, k)
    wi = parse_pair(cur, prop)
    wr.check(wi.current, wi.target, k, res.wave, res.n_waves, res.lower_bound)
    assert res.n_waves == wr.ilp_min_waves(wi.current, wi.target, k) == [4, 2, 1][k - 1]
    assert res.optimal == (k > 1)
    assert sorted((e["partition"], e["replicas"]) for d in res.waves for e in d["partitions"]) == \
        sorted((e["partition"], e["replicas"]) for e in prop["partitions"])


def test_random_small_instances_reach_the_ilp_optimum(kao):
    for s in range(40):
        cur, tgt, k = wr.random_instance(s)
        B = int(max(cur.max(), tgt.max())) + 1
        wave, nw, lb = _valid(cur, tgt, B, k, seed=s + 1)
        assert nw == wr.ilp_min_waves(cur, tgt, k), s
        mwave, mnw, mlb = wr.kernel_model(cur, tgt, k, s + 1)
        assert (wave.tolist(), nw, lb) == (mwave.tolist(), mnw, mlb), s


@pytest.mark.parametrize("k", [1, 2, 5])
def test_config4_cluster_wide(kao, k):
    cur, tgt, B = wr.config4_pair()
    wave, nw, lb = _valid(cur, tgt, B, k)
    if k == 2:   # the whole kernel, bit for bit, at 10,000 partitions
        mwave, mnw, _ = wr.kernel_model(cur, tgt, k, 1)
        assert wave.tolist() == mwave.tolist() and nw == mnw


def _solved_pair(kao, n_brokers0, n_racks, n_topics, P, removed, added):
    """make_cluster's old assignment (old broker ids) against kao.solve's plan (target ids), every topic in one list."""
    from kafka_assignment_optimizer_amd import synthetic as sy
    topics = sy.make_cluster(n_brokers0, n_racks, n_topics, P, 3, removed, added)
    res = kao.solve(topics, seed=1, time_limit_s=5.0, stop_at_bound=1)
    rack0 = np.arange(n_brokers0) % n_racks
    cur, tgt = [], []
    for ti, (t, r) in enumerate(zip(topics, res)):
        assert r.status in ("OPTIMAL_PROVEN", "FEASIBLE_BOUND_GAP", "TIME_LIMIT"), r.status
        cur.append(sy.balanced_fill(n_brokers0, n_racks, P, 3, ti, rack0).astype(np.int64))
        tgt.append(np.asarray(t.broker_ids)[np.asarray(r.assignment, dtype=np.int64).reshape(P, 3)])
    B = n_brokers0 + len(added)
    return np.concatenate(cur).astype(np.uint16), np.concatenate(tgt).astype(np.uint16), B


@pytest.mark.parametrize("k", [1, 2, 5])
def test_decommission_and_expansion(kao, k):
    """Decommission: broker 17 of 100 leaves, its partitions are copied from it while it is still the leader.  Expansion: 6
    brokers join a 60-broker cluster and the bands pull replicas onto them."""
    cur, tgt, B = _solved_pair(kao, 100, 4, 1, 256, [17], [])
    assert 17 in cur and 17 not in tgt
    _valid(cur, tgt, B, k)
    cur, tgt, B = _solved_pair(kao, 60, 3, 4, 64, [], [(60 + i, i % 3) for i in range(6)])
    assert (tgt >= 60).any()
    _valid(cur, tgt, B, k)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_drift100k(kao, k):
    cur, tgt, B = wr.drift100k_pair()
    _valid(cur, tgt, B, k)


def test_deterministic(kao):
    cur, tgt, B = wr.config4_pair()
    a = _run(cur, tgt, B, 2, seed=7)
    b = _run(cur, tgt, B, 2, seed=7)
    assert a[0].tolist() == b[0].tolist() and a[1:] == b[1:]


def test_edge_cases(kao):
    cur = np.array([[0, 1], [1, 2], [2, 0]], dtype=np.uint16)
    # nothing changed
    wave, nw, lb = _run(cur, cur, 3, 1)
    assert (wave.tolist(), nw, lb) == ([-1, -1, -1], 0, 0)
    # order changes only (preferred-leader moves): one wave, no cap counted
    tgt = cur.copy()
    tgt[0] = [1, 0]
    tgt[2] = [0, 2]
    wave, nw, lb = _run(cur, tgt, 3, 1)
    assert (wave.tolist(), nw, lb) == ([0, -1, 0], 1, 1)
    # replica removal only (RF 2 -> 1) moves no data either
    wave, nw, lb = _run(cur, np.array([[0, NONE], [1, 2], [2, 0]], dtype=np.uint16), 3, 1)
    assert (wave.tolist(), nw, lb) == ([0, -1, -1], 1, 1)
    # broker 3 is decommissioned (in no target row) and leads three partitions: it is the source of all three copies
    cur = np.array([[3, 0], [3, 1], [3, 2]], dtype=np.uint16)
    tgt = np.array([[0, 1], [1, 2], [2, 0]], dtype=np.uint16)
    wave, nw, lb = _valid(cur, tgt, 4, 1)
    assert (sorted(wave.tolist()), nw, lb) == ([0, 1, 2], 3, 3)
    wave, nw, lb = _valid(cur, tgt, 4, 3)
    assert (wave.tolist(), nw, lb) == ([0, 0, 0], 1, 1)
    # a metadata-only partition next to moving ones sits in wave 0 and never opens a wave of its own
    cur = np.array([[0, 1], [0, 2], [4, 5]], dtype=np.uint16)
    tgt = np.array([[0, 3], [0, 3], [5, 4]], dtype=np.uint16)
    wave, nw, lb = _valid(cur, tgt, 6, 1)
    assert (nw, lb, wave[2]) == (2, 2, 0)


def test_kao_waves_cli_end_to_end(kao, tmp_path):
    """cli/kao-waves on the README pair (and the Python twin, same files): each wave file is a reassignment document of its
    own, and together they hold exactly the changed partitions with their target replicas."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    cur_path, plan_path = os.path.join(GOLDEN, "readme_current.json"), os.path.join(GOLDEN, "readme_proposal.json")
    prop = load_golden("readme_proposal.json")
    for k, expect in ((1, 4), (2, 2)):
        prefix = str(tmp_path / f"cpp{k}_")
        r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", cur_path, "--plan", plan_path, "--max-per-broker", str(k),
                            "--out-prefix", prefix, "--report"], capture_output=True)
        assert r.returncode == 0, r.stderr
        assert f"waves={expect} lower_bound={[3, 2][k - 1]}".encode() in r.stderr
        docs = [json.load(open(f"{prefix}{w + 1}.json")) for w in range(expect)]
        assert not os.path.exists(f"{prefix}{expect + 1}.json")
        got = []
        for d in docs:
            assert d["version"] == 1 and d["partitions"]
            got += [(e["topic"], e["partition"], e["replicas"]) for e in d["partitions"]]
        assert sorted(got) == sorted((e["topic"], e["partition"], e["replicas"]) for e in prop["partitions"])
        py = str(tmp_path / f"py{k}_")
        r2 = subprocess.run([sys.executable, "-m", "kafka_assignment_optimizer_amd.waves", "--current", cur_path, "--plan", plan_path,
                             "--max-per-broker", str(k), "--out-prefix", py], capture_output=True, cwd=ROOT)
        assert r2.returncode == 0, r2.stderr
        assert [json.load(open(f"{py}{w + 1}.json")) for w in range(expect)] == docs
