"""kao_balance_disk on the MI355X: replica moves that lower the peak of the bytes a broker stores, by synchronous rounds of a
deterministic descent, with a lower bound that proves the peak optimal where the two meet.  Every instance up
to the mid size is held byte for byte against the restatement of the rounds in tests/disk_ref.py; every result is checked for the
invariants: no move is left, the rack rule holds, the bound recomputed from the input is the reported one, two calls give the same
bytes, dry_run reports the same numbers."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import disk_ref as dr
from conftest import ROOT
from disk_launches import disk_launches

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
    return res.status, res.n_moved, res.bytes_moved, res.peak_before, res.peak_after, res.lower_bound


def _invariants(res, again, dry, rows, size, B, rack_of, R, cap, move_leaders, min_gain, stopped):
    """What holds with or without a restatement to compare against."""
    assert (res.lower_bound, int(res.stats[6])) == dr.lower_bound(rows, size, B, move_leaders)   # from the input
    assert res.lower_bound <= res.peak_after <= res.peak_before
    assert res.status == ("OPTIMAL_PROVEN" if res.peak_after == res.lower_bound else "FEASIBLE_BOUND_GAP")
    out = res.rows.astype(np.int64)
    assert res.peak_after == int(dr.loads(out, size, B).max(initial=0)) and res.peak_before == int(dr.loads(rows, size, B).max(initial=0))
    assert int(dr.loads(out, size, B).sum()) == int(dr.loads(rows, size, B).sum())
    assert (res.n_moved, res.bytes_moved) == dr.set_moves(rows, out, size)
    assert dr.rack_rule_holds(rows, out, rack_of, R, cap)
    assert ((out == NONE) == (rows == NONE)).all() and (move_leaders or (out[:, 0] == rows[:, 0]).all())
    if not stopped:
        assert dr.stable(out, size, B, rack_of, R, cap, move_leaders, min_gain)
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()


def _checked(call, c, cap=None, move_leaders=None, min_gain=0, max_rounds=0):
    """One instance through the GPU against the restatement: bytes, numbers, stats[0..2] and [4..7]; twice, and once with dry_run;
    every invariant.  Returns (result, restatement)."""
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    rows = np.asarray(rows, dtype=np.int64)
    cap = c.get("cap", 0) if cap is None else cap
    ml = c.get("move_leaders", True) if move_leaders is None else move_leaders
    ref = dr.descend(rows, size, B, rack_of, R, cap, ml, min_gain, max_rounds)
    res = call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds)
    again = call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds)
    dry = call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, dry_run=True)
    print(f"B={B} P={len(rows)} cap={cap} leaders={ml} gpu={_numbers(res)} stats={res.stats.tolist()} ref rounds={ref['rounds']} moves={ref['moves']} "
          f"proposals={ref['proposals']}")
    assert res.rows.astype(np.int64).tobytes() == ref["rows"].tobytes()
    assert _numbers(res)[1:5] == (ref["n_moved"], ref["bytes_moved"], ref["peak_before"], ref["peak_after"])
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[4] == ref["rows_changed"] and res.stats[5] == int(ref["more"]) and res.stats[7] == ref["brokers_changed"]
    _invariants(res, again, dry, rows, size, B, rack_of, R, cap, ml, min_gain, ref["more"])
    return res, ref


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_matches_the_restatement(call):
    proven = moved = 0
    for seed in range(120):
        res, _ = _checked(call, dr.small_case(seed))
        proven += res.status == "OPTIMAL_PROVEN"
        moved += res.n_moved > 0
    print(f"proven optimal: {proven} of 120, moved: {moved}")
    assert moved >= 60


# ---- 2. contention -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 5, 9])
def test_every_proposal_leaves_one_of_three_sources(call, B):
    """Every replica on brokers 0..2.  Equal sizes: every key ties down to p.  Sizes of 2^40 + a little: the loads pass 2^32 and 2^48."""
    for P in (64, 257, 1500):
        for base in (0, 2 ** 40):
            res, ref = _checked(call, dr.crowded_case(B, P, base=base))
            assert res.n_moved > 0 and res.stats[0] * (B // 2) >= res.stats[1] >= res.n_moved   # winners share no broker: at most B / 2 a round
            if base:
                assert res.peak_before == int(np.sum(dr.crowded_case(B, P, base=base)["size"])) > 2 ** 40 * P >= 2 ** 46 and (P < 257 or res.peak_before > 2 ** 48)
    c = dr.crowded_case(B, 257)
    none, _ = _checked(call, c, min_gain=257 * 5)   # no gap is that large
    assert none.n_moved == 0 and none.stats[0] == 0 and none.stats[5] == 0
    huge, _ = _checked(call, c, min_gain=2 ** 64 - 1)
    assert huge.n_moved == 0 and huge.stats[0] == 0
    one, ref = _checked(call, c, max_rounds=1)
    assert one.stats[0] == 1 and one.stats[5] == 1 and ref["more"]
    kept, _ = _checked(call, c, move_leaders=False)
    assert kept.n_moved > 0 and kept.lower_bound >= 5 * (257 // 3)   # a third of the rows lead from each source


# ---- 3. racks ------------------------------------------------------------------------------------------------------------------------
def test_rack_rule(call):
    rng = np.random.default_rng(3)
    B, R, P = 12, 3, 40
    rack_of = np.arange(B) % R
    rows = np.stack([rng.permutation(R) + R * rng.integers(0, 2, R) for _ in range(P)]).astype(np.int64)   # one replica per rack
    c = dict(rows=rows, size=rng.integers(1, 100, P), B=B, rack_of=rack_of, R=R)
    res, _ = _checked(call, c, cap=1)
    out = res.rows.astype(np.int64)
    assert res.n_moved > 0 and (rack_of[out] == rack_of[rows]).all()   # every move stays inside its rack
    assert (dr.rack_counts(out, rack_of, R) == dr.rack_counts(rows, rack_of, R)).all()
    flat = dict(c, rack_of=np.zeros(B, dtype=np.int64), R=1)   # one rack, cap 1, width 3: the rows start over the cap
    res, _ = _checked(call, flat, cap=1)
    free, _ = _checked(call, flat, cap=0)
    assert res.n_moved > 0 and res.rows.tobytes() == free.rows.tobytes()   # same-rack moves are all there is
    full = dict(rows=np.array([[2, 0, 1, 3], [0, 1, NONE, NONE], [0, 2, NONE, NONE]]), size=[50, 1, 1], B=4, rack_of=np.zeros(4, dtype=np.int64), R=1)
    res, _ = _checked(call, full)
    assert res.rows[0].tolist() == [2, 0, 1, 3]   # a partition on every broker never moves


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------
def test_edge_cases(call):
    res = call(np.zeros((0, 3)), 4, [0, 1, 0, 1], 2, np.zeros(0, dtype=np.int64))   # no partition
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0, 0) and res.stats[[0, 1, 2, 4, 5, 6, 7]].tolist() == [0] * 7
    res, _ = _checked(call, dict(rows=np.zeros((5, 1)), size=[3, 0, 4, 1, 9], B=1, rack_of=[0], R=1))   # one broker
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 17, 17, 17) and res.stats[6] == 1
    rng = np.random.default_rng(8)
    c = dict(rows=dr.skewed_rows(rng, 20, 50, 8, pad=0.6), size=rng.integers(1, 1000, 50), B=20, rack_of=np.arange(20) % 4, R=4)   # width 8, mixed k_p
    assert len({int(k) for k in (c["rows"] != NONE).sum(axis=1)}) >= 5
    for cap, ml in ((0, True), (2, True), (2, False)):
        res, _ = _checked(call, c, cap=cap, move_leaders=ml)
        assert res.n_moved > 0
    res, _ = _checked(call, dict(c, size=np.zeros(50, dtype=np.int64)))   # nothing weighs anything
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0, 0) and res.stats[0] == 0
    top = np.array([[7999, 0, 7], [7999, 7998, NONE], [7999, 9, 7998], [7999, NONE, NONE]])   # KAO_DISK_MAX_BROKERS brokers, the last index in use
    res, _ = _checked(call, dict(rows=top, size=[10, 20, 30, 5], B=8000, rack_of=np.arange(8000) % 255, R=255), cap=1)
    assert res.peak_after == 30 and res.status == "OPTIMAL_PROVEN"


def test_invalid_arguments_leave_the_rows_alone(kao):
    """Every refusal of include/kao.h is one on a machine with a device too."""
    import test_disk_errors as host
    for what, change, code, text in host.REFUSED:
        rc, msg = host._call(**change)
        assert rc == code and text in msg, what


# ---- 5. the mid instance against the restatement -------------------------------------------------------------------------------------
def test_mid_instance_matches_the_restatement(call):
    """60 brokers in 6 racks, 1,500 partitions at RF 3, skewed placement: several workgroups, and enough rounds for the host to read
    the proposal counts more than twice."""
    c = dr.lognormal_case(60, 6, 1500, 3, 0.7, 11)
    res, ref = _checked(call, c, cap=1)
    assert ref["rounds"] > 64 and res.stats[3] > 3 and res.stats[3] >= 3 * ref["rounds"]
    assert res.peak_after < res.peak_before


# ---- 6. a larger instance: invariants only -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move_leaders", [True, False])
def test_larger_instance_keeps_the_invariants(call, move_leaders):
    c = dr.lognormal_case(300, 10, 6000, 3, 0.7, 5)
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    res, again, dry = (call(rows, B, rack_of, R, size, 1, move_leaders, dry_run=d) for d in (False, False, True))
    print(f"leaders={move_leaders} gpu={_numbers(res)} stats={res.stats.tolist()}")
    _invariants(res, again, dry, rows, size, B, rack_of, R, 1, move_leaders, 0, False)
    assert res.peak_after < res.peak_before and res.stats[5] == 0 and res.stats[1] >= res.n_moved > 0
    assert res.stats[4] == int((res.rows.astype(np.int64) != rows).any(axis=1).sum())


# ---- 7. the plan goes on into the wave planner ---------------------------------------------------------------------------------------
def test_plan_feeds_the_wave_planner(call):
    from kafka_assignment_optimizer_amd.waves import plan_waves_sized_arrays
    c = dr.lognormal_case(12, 3, 80, 3, 0.7, 2)
    rows = c["rows"]
    res = call(rows, 12, c["rack_of"], 3, c["size"], 1)
    out = res.rows.astype(np.int64)
    assert res.n_moved > 0
    wave, n_waves, _ = plan_waves_sized_arrays(rows.astype(np.uint16), res.rows, 12, c["size"].astype(np.uint64), int(c["size"].max()) * 3)
    fresh = np.array([len(set(y) - set(x)) > 0 for x, y in zip(rows.tolist(), out.tolist())])
    assert fresh.any() and (np.asarray(wave)[fresh] >= 0).all() and n_waves >= 1


# ---- 8. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"])


def _both(args, tmp_path, tag):
    """Each tool in a fresh child process: the same --out document and the same report."""
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"{tag}{i}.json"
        r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    report = outs[0][1].splitlines()
    assert len(report) == 1 and report[0].startswith("disk: status=")
    return json.loads(outs[0][0]), report[0]


def test_cli_on_the_readme_example(kao, tmp_path):
    """The README topic with its log-dir sizes: every broker holds one replica, so no move helps, the largest partition is the
    proven peak and the plan is empty; both tools say so in the same bytes."""
    from kafka_assignment_optimizer_amd.waves import parse_sizes
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    golden = os.path.join(ROOT, "tests", "golden")
    base = ["--current", os.path.join(golden, "readme_current.json"), "--broker-list", ",".join(str(b) for b in range(20)), "--racks",
            os.path.join(golden, "readme_racks.json"), "--sizes", os.path.join(golden, "readme_log_dirs.txt")]
    sizes = parse_sizes(open(os.path.join(golden, "readme_log_dirs.txt")).read())
    top, total = max(sizes.values()), 2 * sum(sizes.values())
    for tag, flags in (("plain", []), ("rack", ["--max-per-rack", "1", "--keep-leaders"])):
        plan, report = _both(base + flags, tmp_path, tag)
        assert plan == {"version": 1, "partitions": []}
        assert report == (f"disk: status=OPTIMAL_PROVEN peak_before={top} peak_after={top} lower_bound={top} bound_term=largest_partition replicas_moved=0 "
                          f"bytes_moved=0 bytes_total={total} rows_changed=0 brokers_changed=0 rounds=0 moves=0 launches=100")


def test_cli_end_to_end(kao, tmp_path):
    """cli/kao-disk and the Python twin on a three-topic document of mixed RF whose replicas crowd a third of the brokers: the same
    bytes, a plan of the changed rows only, which is the library's; kao-waves takes the plan as it is."""
    from kafka_assignment_optimizer_amd.disk import balance_disk
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(7)
    B, ids = 9, [100 + 3 * i for i in range(9)]
    racks = {b: f"r{i % 3}" for i, b in enumerate(ids)}
    doc, logdirs = {"version": 1, "partitions": []}, {}
    for name, P, rf in (("alpha", 12, 3), ("be-ta", 9, 2), ("gamma", 7, 1)):
        for p in range(P):
            r = rng.permutation(4)[:rf] if rng.random() < 0.8 else rng.permutation(B)[:rf]   # brokers 0..3 hold most of it
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
            w = int(rng.integers(1, 1000))
            if not (name == "gamma" and p == 6):   # one partition is left to --default-size
                for b in r:
                    logdirs.setdefault(ids[b], []).append({"partition": f"{name}-{p}", "size": w * 1024 - int(b), "offsetLag": 0, "isFuture": False})
    cur_path, racks_path, sizes_path = (tmp_path / n for n in ("current.json", "racks.json", "logdirs.txt"))
    cur_path.write_text(json.dumps(doc))
    racks_path.write_text(json.dumps({str(b): r for b, r in racks.items()}))
    sizes_path.write_text("Querying brokers for log directories information\n" + json.dumps(
        {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": "/d", "error": None, "partitions": e}]} for b, e in sorted(logdirs.items())]}) + "\n")
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path), "--sizes", str(sizes_path)]
    for prog in PROGS:   # gamma-6 has no size; usage errors exit with 2
        r = subprocess.run(prog + base + ["--out", str(tmp_path / "x.json")], capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"no size for partitions gamma-6 " in r.stderr, (prog, r.stderr)
        assert subprocess.run(prog + base + ["--default-size", "1K"], capture_output=True, cwd=ROOT).returncode == 2   # no --out
        for bad in (["--min-gain", "1X"], ["--max-rounds", "-1"], ["--max-per-rack", "x"], ["--default-size", str(2 ** 53 + 1)], ["--scope", "rack"]):
            assert subprocess.run(prog + base + ["--out", str(tmp_path / "x.json")] + bad, capture_output=True, cwd=ROOT).returncode == 2, bad
    base += ["--default-size", "70K"]
    for tag, flags, kw in (("plain", [], {}), ("rack", ["--max-per-rack", "1", "--keep-leaders", "--min-gain", "1K"], dict(max_per_rack=1, move_leaders=False, min_gain=1024)),
                           ("one", ["--max-rounds", "1"], dict(max_rounds=1)), ("dry", ["--dry-run"], dict(dry_run=True))):
        plan, report = _both(base + flags, tmp_path, tag)
        lib = balance_disk(doc, sizes_path.read_text(), broker_list=ids, racks=racks, default_size=70 * 1024, **kw)
        res = lib.result
        assert lib.size[lib.input.keys.index(("gamma", 6))] == 70 * 1024
        assert plan == lib.document and len(plan["partitions"]) == (0 if tag == "dry" else res.stats[4])
        assert report.startswith(f"disk: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} lower_bound={res.lower_bound} ")
        assert f" replicas_moved={res.n_moved} bytes_moved={res.bytes_moved} " in report and f" rounds={res.stats[0]} moves={res.stats[1]} " in report
        assert res.peak_after < res.peak_before and res.n_moved > 0
        if tag == "rack":
            cur = {(e["topic"], e["partition"]): e["replicas"] for e in doc["partitions"]}
            assert all(e["replicas"][0] == cur[(e["topic"], e["partition"])][0] for e in plan["partitions"])   # the leaders stay
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", str(cur_path), "--plan", str(tmp_path / "plain0.json"), "--sizes", str(sizes_path),
                        "--default-size", "70K", "--max-bytes-per-broker", "1M", "--out-prefix", str(tmp_path / "wave")], capture_output=True, cwd=ROOT)
    assert r.returncode == 0 and (tmp_path / "wave1.json").exists(), r.stderr


# ---- 9. the ends of a batch of rounds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,max_rounds,rounds,stopped", [(25, 0, 128, 0), (1, 0, 127, 0), (11, 0, 129, 0), (25, 31, 31, 1), (25, 32, 32, 1), (25, 33, 33, 1),
                                                            (25, 64, 64, 1), (25, 128, 128, 0), (25, 129, 128, 0)])
def test_descent_ends_and_max_rounds_on_batch_boundaries(call, seed, max_rounds, rounds, stopped):
    """24 brokers in 4 racks, 400 partitions, one replica per rack.  The host enqueues 32 rounds between two reads of the proposal
    counts: seed 25 takes 128 rounds (the empty round is the first of a fifth batch), seed 1 takes 127 (the last of the fourth), seed 11
    takes 129.  On seed 25 max_rounds falls before, on and after the end of a batch; 128 ends through the probe that finds nothing
    left, 129 by the empty round.  stats[3] is the launch schedule of tests/disk_launches.py."""
    res, ref = _checked(call, dr.lognormal_case(24, 4, 400, 3, 0.7, seed), cap=1, max_rounds=max_rounds)
    assert (ref["rounds"], int(ref["more"])) == (rounds, stopped)
    assert res.stats[3] == disk_launches(rounds, max_rounds, bool(stopped))
