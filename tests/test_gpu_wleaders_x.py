"""kao_balance_leaders_weighted_exchange on the MI355X: the weighted leader balance that goes on from a
move-stable state by swapping the leaders of two partitions on one broker pair.  Every instance is held bit for bit against the
restatement in tests/wleaders_x_ref.py (which asserts the definition's claims every round): rows, every reported number, stats[0..2],
[5], [7] and [8..11]; peak_after is never above kao_balance_leaders_weighted's on the same device; two calls give the same bytes;
dry_run reports the same numbers and leaves the rows alone; the end state is move-stable and, against all pairs, exchange-stable."""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wleaders_ref as wr
import wleaders_x_ref as xr
from conftest import ROOT

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
ONE, MULTI = 1, 2
BOTH = pytest.mark.parametrize("path", [ONE, MULTI], ids=["one", "multi"])


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
    from kafka_assignment_optimizer_amd import _ffi
    was = _ffi.load().kao_wleaders_test_path(path)
    assert was >= 0
    try:
        yield
    finally:
        _ffi.load().kao_wleaders_test_path(was)


def _numbers(res):
    return res.status, res.n_changed, res.peak_before, res.peak_after, res.lower_bound


def _checked(call, rows, weight, B, min_gain=0, max_rounds=0, path=None, ref=None):
    """One instance through the GPU against the restatement (computed once per instance: pass `ref` to share it).  Returns
    (result, restatement, the plain call's result)."""
    rows = np.asarray(rows, dtype=np.int64)
    if ref is None:
        ref = xr.descend(rows, weight, B, min_gain, max_rounds)
    with forced(0 if path is None else path):
        res = call(rows, B, weight, min_gain, max_rounds, exchange=True)
        again = call(rows, B, weight, min_gain, max_rounds, exchange=True)
        dry = call(rows, B, weight, min_gain, max_rounds, dry_run=True, exchange=True)
        plain = call(rows, B, weight, min_gain, max_rounds)
    print(f"B={B} P={len(rows)} gpu={_numbers(res)} stats={res.stats.tolist()} plain peak={plain.peak_after} ref x_rounds={ref['x_rounds']} "
          f"exchanges={ref['exchanges']} x_proposals={ref['x_proposals']} entries={ref['entries']}")
    assert res.stats.shape == (12,) and res.exchange and (res.exchange_rounds, res.exchanges) == (res.stats[8], res.stats[9])
    assert res.rows.astype(np.int64).tobytes() == ref["rows"].tobytes()
    assert (res.n_changed, res.peak_before, res.peak_after) == (ref["n_changed"], ref["peak_before"], ref["peak_after"])
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[5] == int(ref["more"]) and res.stats[7] == ref["leading"]
    assert res.stats[8:].tolist() == [ref["x_rounds"], ref["exchanges"], ref["x_proposals"], ref["entries"]]
    assert (res.lower_bound, int(res.stats[6])) == wr.lower_bound(res.rows, weight, B)
    assert res.lower_bound <= res.peak_after <= plain.peak_after <= res.peak_before == plain.peak_before
    assert res.status == ("OPTIMAL_PROVEN" if res.peak_after == res.lower_bound else "FEASIBLE_BOUND_GAP")
    if not ref["more"]:
        assert wr.stable(rows, res.rows, weight, B, min_gain)
        if len(rows) <= 400:
            assert xr.exchange_stable(res.rows, weight, B, min_gain)
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()
    if path is not None:
        assert res.stats[4] == (1 if path == ONE else 0) == plain.stats[4]
    return res, ref, plain


# ---- 1. the small family on each forced path ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_ref(seed):
    rows, weight, B = wr.small_case(seed)
    return rows, weight, B, xr.descend(rows, weight, B)


@BOTH
def test_small_family_matches_the_restatement(call, path):
    lower = swaps = 0
    for seed in range(120):
        rows, weight, B, ref = _small_ref(seed)
        res, _, plain = _checked(call, rows, weight, B, path=path, ref=ref)
        lower += res.peak_after < plain.peak_after
        swaps += int(res.stats[9])
    print(f"strictly lower than the plain call: {lower} of 120, exchanges: {swaps}")
    assert lower >= 1 and swaps >= 1


# ---- 2. one segment: two brokers, every partition on both -------------------------------------------------------------------------
def _two_brokers(P, seed=3):
    rng = np.random.default_rng(seed)
    rows = np.tile(np.array([0, 1], dtype=np.int64), (P, 1))
    flip = rng.random(P) < 0.3
    rows[flip] = rows[flip][:, ::-1]
    return rows, rng.integers(1, 1000, P).astype(np.int64)


@pytest.mark.parametrize("P,path", [(2, ONE), (2, MULTI), (64, ONE), (64, MULTI), (65, ONE), (65, MULTI), (4097, None)])
def test_two_brokers_are_one_segment(call, P, path):
    rows, weight = _two_brokers(P)
    res, ref, _ = _checked(call, rows, weight, 2, path=path)
    assert res.stats[11] == P
    if P == 4097:
        assert res.stats[4] == 0 and res.stats[3] > 10   # above 4,096 partitions the size picks the multi-launch path
    if P >= 64:
        assert res.stats[9] > 0


# ---- 3. widths, padding, zero weights -------------------------------------------------------------------------------------------
@BOTH
def test_width_two(call, path):
    rows, weight = wr.lognormal_case(8, 300, 2, 0.7, 3)
    res, _, _ = _checked(call, rows, weight, 8, path=path)
    assert res.stats[9] > 0 and res.stats[11] == 300


@BOTH
def test_width_eight_with_full_rows(call, path):
    rng = np.random.default_rng(5)
    rows = np.array([rng.permutation(12)[:8] for _ in range(200)], dtype=np.int64)
    weight = np.maximum(1, np.round(np.exp(rng.normal(10.0, 0.7, 200)))).astype(np.int64)
    res, _, _ = _checked(call, rows, weight, 12, path=path)
    assert res.stats[11] == 200 * 28 and res.stats[9] > 0


@BOTH
def test_padded_rows_and_zero_weights_inside_segments(call, path):
    rng = np.random.default_rng(9)
    rows = wr.skewed_rows(rng, 10, 150, 4, pad=0.5)
    weight = rng.integers(1, 5000, 150).astype(np.int64)
    assert ((rows != NONE).sum(axis=1) == 1).any()
    res, _, _ = _checked(call, rows, weight, 10, path=path)
    assert res.stats[9] > 0
    weight[::3] = 0
    res, ref, _ = _checked(call, rows, weight, 10, path=path)
    held = (rows != NONE).sum(axis=1)
    assert res.stats[11] == int((held * (held - 1) // 2)[weight > 0].sum())


@BOTH
def test_equal_weights_give_the_plain_call_s_bytes(call, path):
    rows, _, B = wr.small_case(4)
    big, _ = wr.lognormal_case(20, 500, 3, 0.7, 2)
    for r, nb in ((rows, B), (big, 20)):
        res, _, plain = _checked(call, r, np.full(len(r), 7, dtype=np.int64), nb, path=path)
        assert res.stats[9] == 0 and res.stats[8] == 0
        assert res.rows.tobytes() == plain.rows.tobytes() and _numbers(res) == _numbers(plain) and res.stats[:8].tolist()[:3] == plain.stats[:3].tolist()


@BOTH
def test_every_proposal_collides_at_one_source(call, path):
    for base in (0, 2 ** 40):
        rows, weight = wr.collide_case(4, 257, base)
        _checked(call, rows, weight, 4, path=path)


# ---- 4. the mid instance down both paths -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mid():
    rows, weight = wr.lognormal_case(30, 3000, 3, 0.7, 7)
    return rows, weight, xr.descend(rows, weight, 30)


def test_mid_instance_gives_the_same_bytes_on_both_paths(call):
    rows, weight, ref = _mid()
    a, _, plain = _checked(call, rows, weight, 30, path=ONE, ref=ref)
    b, _, _ = _checked(call, rows, weight, 30, path=MULTI, ref=ref)
    assert a.rows.tobytes() == b.rows.tobytes() and _numbers(a) == _numbers(b)
    assert a.stats[[0, 1, 2, 5, 6, 7, 8, 9, 10, 11]].tolist() == b.stats[[0, 1, 2, 5, 6, 7, 8, 9, 10, 11]].tolist()
    assert a.peak_after < plain.peak_after and a.stats[8] > 10
    by_size = call(rows, 30, weight, exchange=True)
    assert by_size.stats[4] == 1   # B <= 2,048 and P <= 4,096: one workgroup


# ---- 5. large weights ----------------------------------------------------------------------------------------------------------------
@BOTH
def test_weights_near_2_60(call, path):
    """Loads pass 2^61, the sum stays below 2^62: 2 weight + D and 2 delta stay inside 64 bits."""
    rng = np.random.default_rng(11)
    rows = np.array([rng.permutation(3)[:2] for _ in range(40)], dtype=np.int64)
    rows[:3] = [[0, 1], [0, 2], [0, 1]]
    weight = rng.integers(1, 2 ** 40, 40).astype(np.int64)
    weight[:3] = [2 ** 60, 2 ** 60 - 12345, 2 ** 60 - 2 ** 33]
    assert 2 ** 61 < int(weight.sum()) < 2 ** 62
    res, _, _ = _checked(call, rows, weight, 3, path=path)
    assert res.peak_before > 2 ** 61


# ---- 6. min_gain ----------------------------------------------------------------------------------------------------------------------
@BOTH
def test_min_gain_above_half_the_gap_still_finds_the_exchange(call, path):
    """The hand-built case of tests/test_wleaders_x_ref.py: the only passing partner is on the heavy side of the split, behind one
    that fails, and 2 min_gain >= D."""
    from test_wleaders_x_ref import forced_case
    rows, weight, B, mg = forced_case()
    res, ref, plain = _checked(call, rows, weight, B, min_gain=mg, path=path)
    assert plain.n_changed == 0 and res.stats[9] == 1 and res.stats[8] == 1 and res.n_changed == 2
    assert res.rows[0].tolist() == [1, 0] and res.rows[3].tolist() == [0, 1] and (res.peak_after, plain.peak_after) == (568, 573)


@BOTH
def test_min_gain_values(call, path):
    rows, weight = wr.lognormal_case(6, 300, 3, 0.7, 7)
    free, _, _ = _checked(call, rows, weight, 6, path=path)
    some, _, _ = _checked(call, rows, weight, 6, min_gain=20000, path=path)
    none, _, _ = _checked(call, rows, weight, 6, min_gain=2 ** 62, path=path)
    assert free.stats[9] > some.stats[9] > 0 and free.peak_after <= some.peak_after
    assert none.n_changed == 0 and none.stats[0] == 0 and none.stats[5] == 0


# ---- 7. max_rounds at its three edges ------------------------------------------------------------------------------------------------
@BOTH
def test_max_rounds_edges(call, path):
    rows, weight = wr.lognormal_case(6, 300, 3, 0.7, 7)
    full = xr.descend(rows, weight, 6)
    moves = wr.descend(rows, weight, 6)["rounds"]   # the first exchange round is round `moves` (counted from 0)
    assert full["x_rounds"] >= 3 and full["rounds"] > moves + 2
    for limit, x_rounds, more in ((moves - 1, 0, 1), (moves, 0, 1), (moves + 1, 1, 1), (full["rounds"] - 1, None, 1), (full["rounds"], full["x_rounds"], 0)):
        res, ref, _ = _checked(call, rows, weight, 6, max_rounds=limit, path=path)
        assert res.stats[0] == limit and res.stats[5] == more, limit
        if x_rounds is not None:
            assert res.stats[8] == x_rounds, limit


# ---- 7b. the rounds against the batches of the multi-launch path (32 rounds between two reads of the counts) -------------------------
@BOTH
def test_last_round_with_a_proposal_is_the_last_of_a_batch(call, path):
    """The descent takes exactly 32 rounds, 13 of them exchange rounds (tests/test_wleaders_x_ref.py holds the generator to it): the
    first batch is full and the first round of the second is empty.  Launches: init and the peak before, two batches of 32 rounds of
    three, rank, finish, scan."""
    rows, weight = wr.lognormal_case(5, 120, 3, 0.7, 28)
    res, _, _ = _checked(call, rows, weight, 5, path=path)
    assert res.stats[0] == 32 and res.stats[5] == 0 and res.stats[8] == 13
    if path == MULTI:
        assert res.stats[3] == 2 + 3 * 64 + 3


@BOTH
def test_max_rounds_at_and_around_a_batch(call, path):
    """Launches on the multi-launch path: the 5 around the rounds, 3 a round and, every one of the max_rounds rounds having had a
    proposal, the probe of 2."""
    rows, weight = wr.lognormal_case(6, 300, 3, 0.7, 7)
    for limit, rounds, more, x_rounds in ((31, 31, 1, 0), (32, 32, 1, 0), (33, 33, 1, 0), (64, 64, 1, 10)):
        res, _, _ = _checked(call, rows, weight, 6, max_rounds=limit, path=path)
        assert (res.stats[0], res.stats[5], res.stats[8]) == (rounds, more, x_rounds), limit
        if path == MULTI:
            assert res.stats[3] == 5 + 3 * limit + 2, limit


# ---- 8. the command-line tools and the Python API ------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"])


def test_cli_and_python_api_end_to_end(kao, tmp_path):
    """Both tools with --exchange on a small document: the same bytes, the second report line, the library's rows; and without the
    flag the plain call's plan.  balance_leaders_weighted(exchange=True) on the same topics."""
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.failover import parse_current
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_weighted, balance_leaders_weighted_arrays, parse_traffic, weights_for
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rows, weight = wr.lognormal_case(5, 60, 3, 0.7, 7)
    ids = [10 + 2 * b for b in range(5)]
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": p, "replicas": [ids[b] for b in r]} for p, r in enumerate(rows.tolist())]}
    traffic = {"version": 1, "partitions": [{"topic": "t", "partition": p, "weight": int(w)} for p, w in enumerate(weight)]}
    (tmp_path / "current.json").write_text(json.dumps(doc))
    (tmp_path / "traffic.json").write_text(json.dumps(traffic))
    racks = {b: f"r{i % 2}" for i, b in enumerate(ids)}
    base = ["--current", str(tmp_path / "current.json"), "--broker-list", ",".join(str(b) for b in ids), "--racks",
            ",".join(f"{b}:{r}" for b, r in racks.items()), "--traffic", str(tmp_path / "traffic.json"), "--report"]
    fi = parse_current(doc, ids, racks)
    w = weights_for(fi.keys, parse_traffic(traffic))
    plans = {}
    for flag in ([], ["--exchange"]):
        outs = []
        for i, prog in enumerate(PROGS):
            out = tmp_path / f"plan{len(flag)}{i}.json"
            r = subprocess.run(prog + base + flag + ["--out", str(out)], capture_output=True, cwd=ROOT)
            assert r.returncode == 0, r.stderr
            outs.append((out.read_bytes(), r.stderr.decode()))
        assert outs[0] == outs[1]
        res = balance_leaders_weighted_arrays(fi.rows, 5, w, exchange=bool(flag))
        report = outs[0][1].splitlines()
        assert len(report) == 1 + len(flag) and report[0].startswith("weighted: status=") and f"peak_after={res.peak_after} " in report[0]
        if flag:
            assert report[1] == f"exchange: rounds={res.stats[8]} exchanges={res.stats[9]} proposals={res.stats[10]} pair_index_entries={res.stats[11]}"
            assert res.stats[9] > 0
        plans[bool(flag)] = (json.loads(outs[0][0]), res)
        assert len(plans[bool(flag)][0]["partitions"]) == res.n_changed
        after = {e["partition"]: e["replicas"] for e in plans[bool(flag)][0]["partitions"]}
        assert [after.get(p, [ids[b] for b in r]) for p, r in enumerate(rows.tolist())] == [[ids[b] for b in r] for r in res.rows.tolist()]
    assert plans[True][1].peak_after < plans[False][1].peak_after and plans[True][1].n_changed > plans[False][1].n_changed
    ref = xr.descend(fi.rows, w, 5)
    assert plans[True][1].rows.astype(np.int64).tobytes() == ref["rows"].tobytes()
    t = Topic(name="t", broker_ids=np.array(ids), rack_of=np.arange(5) % 2, n_racks=2, n_partitions=60, rf=3, current=rows.astype(np.uint16))
    plan = balance_leaders_weighted([t], [weight], exchange=True)
    assert plan.result.exchange and plan.result.rows.tobytes() == plans[True][1].rows.tobytes() and len(plan.entries) == plan.result.n_changed
    assert plan.result.exchanges == ref["exchanges"] and plan.result.exchange_rounds == ref["x_rounds"]
    dry = balance_leaders_weighted([t], [weight], exchange=True, dry_run=True)
    assert dry.entries == [] and _numbers(dry.result) == _numbers(plan.result)
