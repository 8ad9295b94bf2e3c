"""kao_balance_disk_drain on the MI355X: disk-usage balance with brokers that are to end empty.  Every instance
is held byte for byte against the restatement of the rounds in tests/disk_drain_ref.py: rows, all numbers, stats[0..2] and [4..9];
every case runs twice and once with dry_run, and is checked for the invariants: every replica left is stranded, no move among the
live brokers is left, the rack rule holds, nothing arrives on a draining broker.  Without a draining broker the call is
kao_balance_disk, launch for launch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import disk_drain_ref as dd
import disk_ref as dr
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
    from kafka_assignment_optimizer_amd.disk import balance_disk_arrays
    return balance_disk_arrays


def _numbers(res):
    return res.status, res.n_moved, res.bytes_moved, res.peak_before, res.peak_after, res.lower_bound, res.n_left, res.bytes_left


def _checked(call, c, drain, cap=None, move_leaders=None, min_gain=0, max_rounds=0):
    """One instance through the GPU against the restatement: bytes, numbers, stats[0..2] and [4..9]; twice, and once with dry_run;
    every invariant.  Returns (result, restatement)."""
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    rows = np.asarray(rows, dtype=np.int64)
    size = np.asarray(size, dtype=np.int64)
    drain = np.asarray(drain, dtype=np.uint8)
    cap = c.get("cap", 0) if cap is None else cap
    ml = c.get("move_leaders", True) if move_leaders is None else move_leaders
    ref = dd.descend_drain(rows, size, B, rack_of, R, drain, cap, ml, min_gain, max_rounds)
    res, again, dry = (call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, dry_run=d, drain=drain) for d in (False, False, True))
    print(f"B={B} P={len(rows)} D={int(drain.sum())} cap={cap} leaders={ml} gpu={_numbers(res)} stats={res.stats.tolist()} ref rounds={ref['rounds']} "
          f"moves={ref['moves']} proposals={ref['proposals']} drain_moves={ref['drain_moves']} last={ref['last_drain_round']}")
    out = res.rows.astype(np.int64)
    assert out.tobytes() == ref["rows"].tobytes()
    bound, term = dd.lower_bound_drain(rows, size, B, drain, ml)
    assert _numbers(res)[1:] == (ref["n_moved"], ref["bytes_moved"], ref["peak_before"], ref["peak_after"], bound, ref["n_left"], ref["bytes_left"])
    assert res.status == ("OPTIMAL_PROVEN" if ref["n_left"] == 0 and ref["peak_after"] == bound else "FEASIBLE_BOUND_GAP")
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[4:].tolist() == [ref["rows_changed"], int(ref["more"]), term, ref["brokers_changed"], ref["drain_moves"], ref["last_drain_round"]]
    assert (res.drain_moves, res.last_drain_round) == (ref["drain_moves"], ref["last_drain_round"])
    # what holds with or without a restatement
    assert (res.n_left, res.bytes_left) == dd.left_on(out, size, drain) and res.n_left + res.drain_moves == dd.left_on(rows, size, drain)[0]
    assert res.peak_after == int(dr.loads(out, size, B).max(initial=0)) and res.peak_before == int(dr.loads(rows, size, B).max(initial=0))
    assert (res.n_moved, res.bytes_moved) == dr.set_moves(rows, out, size) and dr.rack_rule_holds(rows, out, rack_of, R, cap)
    assert ((out == NONE) == (rows == NONE)).all()
    on = (out != NONE) & (drain[np.where(out != NONE, out, 0)] != 0)
    assert (out[on] == rows[on]).all()                         # nothing arrived on a draining broker
    if len(rows) and not ml:
        live0 = drain[rows[:, 0]] == 0
        assert (out[live0, 0] == rows[live0, 0]).all()         # a leader on a live broker stays
    if not ref["more"]:
        assert dd.left_is_stranded(out, B, rack_of, R, drain, cap) and dd.stable_live(out, size, B, rack_of, R, drain, cap, ml, min_gain)
        assert res.n_left or res.lower_bound <= res.peak_after
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()
    return res, ref


def _flags(B, ids):
    return dd.drain_flags(B, ids)


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_matches_the_restatement(call):
    complete = 0
    for seed in range(120):
        c = dr.small_case(seed)
        res, _ = _checked(call, c, dd.drain_of(seed, c["B"]))
        complete += res.n_left == 0
    print(f"nothing left: {complete} of 120")
    assert complete >= 100


# ---- 2. without a draining broker: kao_balance_disk --------------------------------------------------------------------------------------
def _same_as_plain(call, c, cap, ml):
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    plain = call(rows, B, rack_of, R, size, cap, ml)
    res = call(rows, B, rack_of, R, size, cap, ml, drain=np.zeros(B, dtype=np.uint8))
    assert res.rows.tobytes() == plain.rows.tobytes() and _numbers(res)[:6] == (plain.status, plain.n_moved, plain.bytes_moved, plain.peak_before, plain.peak_after,
                                                                               plain.lower_bound)
    assert res.stats[:8].tolist() == plain.stats.tolist() and res.stats[8:].tolist() == [0, 0] and (res.n_left, res.bytes_left) == (0, 0)
    return res


def test_no_draining_broker_is_the_plain_call(call):
    moved = 0
    for seed in range(120):
        c = dr.small_case(seed)
        moved += _same_as_plain(call, c, c["cap"], c["move_leaders"]).n_moved > 0
    assert moved >= 60
    for ml in (True, False):
        assert _same_as_plain(call, dr.lognormal_case(60, 6, 1500, 3, 0.7, 5), 1, ml).n_moved > 0


# ---- 3. the mid instance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move_leaders", [True, False])
def test_mid_instance_matches_the_restatement(call, move_leaders):
    """60 brokers in 6 racks, 1,500 partitions at RF 3, brokers 7, 31 and 59 draining: several workgroups and several batches of rounds."""
    c = dr.lognormal_case(60, 6, 1500, 3, 0.7, 5)
    res, ref = _checked(call, c, _flags(60, [7, 31, 59]), cap=1, move_leaders=move_leaders)
    assert res.n_left == 0 and res.drain_moves == 248 and ref["rounds"] > 64 and res.last_drain_round >= 64


# ---- 4. edges, the replicas left written out by hand ------------------------------------------------------------------------------------
def _one_rack(rows, size, B):
    return dict(rows=np.array(rows), size=np.array(size, dtype=np.int64), B=B, rack_of=np.zeros(B, dtype=np.int64), R=1)


def test_two_brokers_one_draining_width_one(call):
    res, _ = _checked(call, _one_rack([[0], [0], [1]], [5, 3, 4], 2), [1, 0])
    assert res.n_left == 0 and res.rows.tolist() == [[1], [1], [1]] and res.stats[0] == 2 and (res.peak_before, res.peak_after) == (8, 12)   # the peak rises
    assert res.status == "OPTIMAL_PROVEN" and res.lower_bound == 12


def test_one_live_broker(call):
    """Brokers 0 and 1 drain, 2 stays: row 0 sends one of its two replicas there, row 1 already holds it, row 2 is on it."""
    res, _ = _checked(call, _one_rack([[0, 1], [0, 2], [2, NONE]], [5, 3, 4], 3), [1, 1, 0])
    assert res.n_left == 2 and res.bytes_left == 8 and res.drain_moves == 1 and res.status == "FEASIBLE_BOUND_GAP"


def test_draining_broker_that_holds_nothing(call):
    res, _ = _checked(call, _one_rack([[0, 1], [0, 2], [0, 1], [1, 0]], [5, 3, 4, 9], 4), [0, 0, 0, 1])
    assert res.n_left == 0 and res.drain_moves == 0 and res.last_drain_round == 0 and (res.rows != 3).all()


def test_draining_broker_with_leaders_only_and_leaders_kept(call):
    res, _ = _checked(call, _one_rack([[2, 0], [2, 1], [0, 1], [2, NONE]], [5, 3, 40, 7], 4), [0, 0, 1, 0], move_leaders=False)
    assert res.n_left == 0 and res.drain_moves == 3 and (res.rows != 2).all() and res.rows[2, 0] == 0   # the leader on live broker 0 stays


def test_size_zero_partitions_leave_a_draining_broker(call):
    res, _ = _checked(call, _one_rack([[0, 1], [0, NONE], [1, 0], [2, 1]], [0, 0, 5, 0], 4), [1, 0, 0, 0])
    assert res.n_left == 0 and res.drain_moves == 3 and res.n_moved == 3 and res.bytes_moved == 5 and (res.rows != 0).all()
    assert res.rows[3].tolist() == [2, 1]   # a size-0 partition on live brokers is skipped, as ever


def test_min_gain_of_2_to_the_62_leaves_the_drain_moves_only(call):
    c = dr.lognormal_case(12, 3, 80, 3, 0.7, 2)
    res, _ = _checked(call, c, _flags(12, [0]), min_gain=2 ** 62)
    free, _ = _checked(call, c, _flags(12, [0]))
    held = int((c["rows"] == 0).sum())
    assert res.n_left == 0 and res.stats[1] == res.drain_moves == held and res.n_moved == held and free.stats[1] > free.drain_moves == held


def test_widest_rows_strand_one_replica_each(call):
    """10 brokers, 3 draining, rows of KAO_MAX_RF = 8 = B - D + 1 brokers: a row with d replicas on draining brokers has d - 1 live
    brokers outside it, so exactly one of them stays."""
    rng = np.random.default_rng(4)
    rows = np.stack([rng.permutation(10)[:8] for _ in range(20)])
    res, _ = _checked(call, _one_rack(rows, rng.integers(1, 100, 20), 10), _flags(10, [2, 5, 9]))
    assert res.n_left == 20 and ((res.rows == 2) | (res.rows == 5) | (res.rows == 9)).sum(axis=1).tolist() == [1] * 20 and res.status == "FEASIBLE_BOUND_GAP"


def test_stranded_by_the_rack_rule(call):
    """Racks a | b b, one replica per rack: row 0 = [0, 1] cannot send broker 0's replica to 2, whose rack is at its cap; row 1 can."""
    c = dict(rows=np.array([[0, 1], [0, NONE]]), size=np.array([6, 2]), B=3, rack_of=np.array([0, 1, 1]), R=2)
    res, _ = _checked(call, c, [1, 0, 0], cap=1)
    assert res.n_left == 1 and res.bytes_left == 6 and res.rows[0].tolist() == [0, 1] and res.rows[1, 0] in (1, 2)
    assert dd.stranded_reasons(res.rows, 3, c["rack_of"], 2, [1, 0, 0], 1) == [(0, 0, 0, "rack_rule")]
    free, _ = _checked(call, c, [1, 0, 0], cap=0)
    assert free.n_left == 0


def test_rank_ties_of_two_draining_brokers_go_by_index(call):
    res, _ = _checked(call, _one_rack([[1, 0], [3, 0], [1, 2], [3, 2], [4, NONE]], [7, 7, 7, 7, 1], 5), [0, 1, 0, 1, 0])
    assert res.n_left == 0 and res.drain_moves == 4


@pytest.mark.parametrize("P", [255, 256, 257])
def test_every_row_on_the_draining_broker_across_a_workgroup_boundary(call, P):
    c = _one_rack(np.zeros((P, 1)), 1 + np.arange(P) % 7, 4)
    res, _ = _checked(call, c, [1, 0, 0, 0])
    assert res.n_left == 0 and res.drain_moves == P and res.stats[0] >= P   # one replica a round


def test_crowded_case_with_broker_0_draining(call):
    res, _ = _checked(call, dr.crowded_case(9, 100), _flags(9, [0]))
    assert res.n_left == 0 and res.drain_moves == 100


@pytest.mark.parametrize("max_rounds", [31, 32, 33])
def test_max_rounds_on_a_batch_boundary_leaves_replicas_that_are_not_stranded(call, max_rounds):
    """64 rows on the draining broker need 64 rounds; the host enqueues 32 between two reads of the proposal counts."""
    c = _one_rack(np.zeros((64, 1)), np.full(64, 3), 3)
    res, ref = _checked(call, c, [1, 0, 0], max_rounds=max_rounds)
    assert res.stats[5] == 1 and ref["more"] and res.stats[0] == max_rounds and res.n_left == 64 - max_rounds > 0
    assert not dd.left_is_stranded(res.rows, 3, c["rack_of"], 1, [1, 0, 0])


# ---- 5. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"])


def _both(args, tmp_path, tag, status):
    """Each tool in a fresh child process: the same exit status, the same --out document and the same report."""
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"{tag}{i}.json"
        r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == status, (prog, r.returncode, r.stderr)
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    return json.loads(outs[0][0]), outs[0][1].splitlines()


def test_cli_end_to_end(kao, tmp_path):
    """cli/kao-disk --drain and the Python twin on a two-topic document over nine brokers in three racks: the same bytes; the report
    names the draining brokers and what is left; with a replica stranded by the rack rule the exit status is 3 after every file is
    written; otherwise kao-waves takes the plan and its waves end with nothing on the drained brokers."""
    from kafka_assignment_optimizer_amd.disk import balance_disk
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(9)
    ids = [100 + 3 * i for i in range(9)]
    racks = {b: f"r{i % 3}" for i, b in enumerate(ids)}
    doc, sizes = {"version": 1, "partitions": []}, {"partitions": []}
    for name, P, rf in (("alpha", 14, 3), ("be-ta", 9, 2)):
        for p in range(P):
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in rng.permutation(9)[:rf]]})
            sizes["partitions"].append({"topic": name, "partition": p, "size": int(rng.integers(1, 1000)) * 1024})
    cur_path, racks_path, sizes_path = (tmp_path / n for n in ("current.json", "racks.json", "sizes.json"))
    cur_path.write_text(json.dumps(doc))
    racks_path.write_text(json.dumps({str(b): r for b, r in racks.items()}))
    sizes_path.write_text(json.dumps(sizes))
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path), "--sizes", str(sizes_path)]
    drained = [ids[1], ids[6]]
    plan, report = _both(base + ["--drain", f"{drained[1]},{drained[0]}", "--max-per-rack", "2"], tmp_path, "plan", 0)
    lib = balance_disk(doc, sizes, broker_list=ids, racks=racks, max_per_rack=2, drain=drained)
    res = lib.result
    held = sum(len(set(e["replicas"]) & set(drained)) for e in doc["partitions"])
    assert plan == lib.document and res.n_left == 0 and res.drain_moves == held > 0 and len(report) == 1
    assert report[0].startswith(f"disk: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} lower_bound={res.lower_bound} ")
    assert report[0].endswith(f" draining={drained[0]},{drained[1]} drain_bytes_before={sum(int(lib.size[p]) for p, r in enumerate(lib.input.rows) for b in r if b in (1, 6))} "
                              f"drain_bytes_after=0 drain_moves={held} last_drain_round={res.last_drain_round} replicas_left=0 bytes_left=0")
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", str(cur_path), "--plan", str(tmp_path / "plan0.json"), "--sizes", str(sizes_path),
                        "--max-bytes-per-broker", "2M", "--out-prefix", str(tmp_path / "wave")], capture_output=True, cwd=ROOT)
    assert r.returncode == 0 and (tmp_path / "wave1.json").exists(), r.stderr
    state = {(e["topic"], e["partition"]): e["replicas"] for e in doc["partitions"]}
    i = 1
    while (tmp_path / f"wave{i}.json").exists():
        state.update({(e["topic"], e["partition"]): e["replicas"] for e in json.loads((tmp_path / f"wave{i}.json").read_text())["partitions"]})
        i += 1
    assert not any(set(r) & set(drained) for r in state.values()) and all(len(set(r)) == len(r) for r in state.values())
    # one replica per rack and all of rack r1 draining: a replica there can go only to a rack its row does not hold yet, so the rows
    # that hold r0 and r2 besides keep theirs (the restatement leaves 5 of 16)
    rack1 = [ids[1], ids[4], ids[7]]
    plan, report = _both(base + ["--drain", ",".join(str(b) for b in rack1), "--max-per-rack", "1"], tmp_path, "stuck", 3)
    lib = balance_disk(doc, sizes, broker_list=ids, racks=racks, max_per_rack=1, drain=rack1)
    assert plan == lib.document and lib.result.n_left > 0 and len(report) == 1 + lib.result.n_left
    assert f" replicas_left={lib.result.n_left} bytes_left={lib.result.bytes_left}" in report[0]
    assert report[1:] == [f"disk: left {t}-{p} broker={b} reason={why}" for t, p, b, why in lib.left] and {why for _, _, _, why in lib.left} == {"rack_rule"}
