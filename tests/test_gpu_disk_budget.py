"""kao_balance_disk_budget on the MI355X: the disk-usage balance under a budget of bytes copied.  Every case
is held byte for byte against the restatement in tests/disk_budget_ref.py (rows, n_moved, bytes_moved, the peaks, stats[0..2] and
[4..9]), called twice and once with dry_run, and checked for what holds of every result: the bytes moved stay inside the budget, the
end state is stable under what is left of it, stats[9] says whether it is move-stable without a budget, the rack rule holds."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import disk_budget_ref as br
import disk_ref as dr
from conftest import ROOT
from disk_launches import disk_launches

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
NO_BUDGET = 2 ** 64 - 1


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


def _stored(c):
    """The bytes the cluster stores."""
    return int((np.asarray(c["size"], dtype=np.int64)[:, None] * (np.asarray(c["rows"]) != NONE)).sum())


def _checked(call, c, max_bytes, cap=None, move_leaders=None, min_gain=0, max_rounds=0):
    """One instance through the GPU against the restatement; max_bytes None = no budget (UINT64_MAX in the call).  Returns (result,
    restatement)."""
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    rows = np.asarray(rows, dtype=np.int64)
    cap = c.get("cap", 0) if cap is None else cap
    ml = c.get("move_leaders", True) if move_leaders is None else move_leaders
    budget = NO_BUDGET if max_bytes is None else max_bytes
    ref = br.descend(rows, size, B, rack_of, R, cap, ml, min_gain, max_rounds, max_bytes)
    res, again, dry = (call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, dry_run=d, max_bytes=budget) for d in (False, False, True))
    print(f"B={B} P={len(rows)} cap={cap} leaders={ml} max_bytes={max_bytes} gpu={_numbers(res)} stats={res.stats.tolist()} ref rounds={ref['rounds']} "
          f"moves={ref['moves']} proposals={ref['proposals']} refused={ref['refused']} bound={ref['budget_bound']}")
    out = res.rows.astype(np.int64)
    assert len(res.stats) == 10 and res.max_bytes == budget
    assert out.tobytes() == ref["rows"].tobytes()
    assert _numbers(res)[1:5] == (ref["n_moved"], ref["bytes_moved"], ref["peak_before"], ref["peak_after"])
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[4:].tolist() == [ref["rows_changed"], int(ref["more"]), dr.lower_bound(rows, size, B, ml)[1], ref["brokers_changed"], ref["refused"],
                                      int(ref["budget_bound"])]
    # what holds with or without a restatement
    assert res.bytes_moved <= budget and (res.n_moved, res.bytes_moved) == dr.set_moves(rows, out, size)
    assert res.lower_bound == dr.lower_bound(rows, size, B, ml)[0] <= res.peak_after <= res.peak_before
    assert res.status == ("OPTIMAL_PROVEN" if res.peak_after == res.lower_bound else "FEASIBLE_BOUND_GAP")
    assert res.peak_after == int(dr.loads(out, size, B).max(initial=0)) and dr.rack_rule_holds(rows, out, rack_of, R, cap)
    assert ((out == NONE) == (rows == NONE)).all() and (ml or (out[:, 0] == rows[:, 0]).all())
    if not ref["more"]:
        assert br.stable_budget(out, rows, size, B, rack_of, R, cap, ml, min_gain, budget - res.bytes_moved)
        assert res.stats[9] == int(not dr.stable(out, size, B, rack_of, R, cap, ml, min_gain))
    else:
        assert res.stats[9] == 0
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()
    return res, ref


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _free_bytes(seed):
    """bytes_moved of the unbudgeted restatement: what the budgets of the family are tenths of."""
    c = dr.small_case(seed)
    return dr.descend(c["rows"], c["size"], c["B"], c["rack_of"], c["R"], c["cap"], c["move_leaders"])["bytes_moved"]


@pytest.mark.parametrize("tenths", [0, 1, 3, 6, None], ids=["0", "1/10", "3/10", "6/10", "none"])
def test_small_family_matches_the_restatement(call, tenths):
    binding = refusing = 0
    for seed in range(120):
        c = dr.small_case(seed)
        res, ref = _checked(call, c, None if tenths is None else _free_bytes(seed) * tenths // 10)
        binding += int(res.stats[9])
        refusing += res.stats[8] > 0
        if tenths == 0:
            assert res.n_moved == 0 and res.stats[0] == 0 and (res.rows == c["rows"]).all()
        if tenths is None:   # kao_balance_disk on the same input
            plain = call(c["rows"], c["B"], c["rack_of"], c["R"], c["size"], c["cap"], c["move_leaders"])
            assert len(plain.stats) == 8 and plain.rows.tobytes() == res.rows.tobytes() and _numbers(plain) == _numbers(res)
            assert plain.stats[:3].tolist() == res.stats[:3].tolist() and plain.stats[4:8].tolist() == res.stats[4:8].tolist()
            assert res.stats[8] == 0 and res.stats[9] == 0
    print(f"tenths={tenths}: the budget stops {binding} of 120, {refusing} refuse a winner")
    assert tenths != 0 or binding >= 60   # with no budget at all, every instance that the descent would change


# ---- 2. contention -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,P,base", [(5, 257, 0), (9, 1500, 2 ** 40)])
def test_contention(call, B, P, base):
    """Every replica on brokers 0..2: all proposals of a round have one of three sources, and few of them win."""
    c = dr.crowded_case(B, P, base=base)
    free = dr.descend(c["rows"], c["size"], B, c["rack_of"], 1)["bytes_moved"]
    for tenths in (1, 5):
        res, _ = _checked(call, c, free * tenths // 10)
        assert 0 < res.bytes_moved <= free * tenths // 10 and res.stats[9] == 1


def test_min_gain_and_max_rounds_with_a_budget(call):
    c = dr.crowded_case(5, 257)
    free = dr.descend(c["rows"], c["size"], 5, c["rack_of"], 1)["bytes_moved"]
    res, _ = _checked(call, c, free // 2, min_gain=15)
    assert res.n_moved > 0
    one, ref = _checked(call, c, free // 2, max_rounds=1)
    assert one.stats[0] == 1 and one.stats[5] == 1 and ref["more"] and one.stats[9] == 0
    both, _ = _checked(call, c, free // 10, min_gain=15, max_rounds=1)
    assert both.stats[0] == 1


# ---- 3. racks and leaders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("percent", [2, 10])
def test_racks_and_leaders(call, percent):
    c = dr.lognormal_case(12, 3, 80, 3, 0.7, 2)
    res, _ = _checked(call, c, _stored(c) * percent // 100, cap=1)
    assert res.stats[9] == 1
    rng = np.random.default_rng(8)
    c = dict(rows=dr.skewed_rows(rng, 20, 50, 8, pad=0.6), size=rng.integers(1, 1000, 50), B=20, rack_of=np.arange(20) % 4, R=4)   # width 8, mixed k_p
    res, _ = _checked(call, c, _stored(c) * percent // 100, cap=2, move_leaders=False)
    assert res.n_moved > 0


# ---- 4. several wavefronts of winners ------------------------------------------------------------------------------------------------
def test_several_wavefronts_of_winners(call):
    """600 brokers, 3,000 partitions, a budget of 2 % of the stored bytes: over a hundred winners in a round, sources far past the first
    wavefronts of ranks, and refusals."""
    c = dr.lognormal_case(600, 6, 3000, 3, 0.7, 5)
    res, ref = _checked(call, c, _stored(c) * 2 // 100, cap=1)
    print(f"max winners a round {ref['max_winners']}, top source rank {ref['top_rank']}")
    assert (ref["rounds"], ref["moves"], ref["refused"]) == (21, 116, 53) and ref["max_winners"] == 110 and ref["top_rank"] == 544
    assert res.stats[8] == 53 and res.stats[9] == 1


# ---- 5. the scan across the whole workgroup, in closed form --------------------------------------------------------------------------
@pytest.mark.parametrize("short", [0, 1], ids=["fits", "one-below"])
def test_scan_across_the_workgroup(call, short):
    """8,000 brokers, one rack, width 1; partitions p and p + 3000 on broker p < 3000, sizes 2^20 + 7p and 2^10.  Broker 2999 - r has
    rank r and its large partition wins the way to broker 7999 - r: 3,000 winners in round 1, charges falling with the rank.  With
    the sum of the 1,777 largest (+ 5) as the budget exactly the ranks 0..1776 are applied; one byte below that sum the 1,777th is
    refused, and so is every later one, although a smaller one would fit what is left."""
    B, P = 8000, 6000
    rows = (np.arange(P) % 3000)[:, None]
    size = np.where(np.arange(P) < 3000, 2 ** 20 + 7 * np.arange(P), 2 ** 10).astype(np.int64)
    top = int(np.sort(size)[::-1][:1777].sum())
    n = 1777 - short
    c = dict(rows=rows, size=size, B=B, rack_of=np.zeros(B, dtype=np.int64), R=1)
    res, ref = _checked(call, c, top - 1 if short else top + 5, max_rounds=1)
    # what is left after the round: 5 bytes, which buy nothing, so the budget ends it; or one byte less than the 1,777th size, which
    # still buys every smaller partition, so max_rounds ends it
    assert res.bytes_moved == int(np.sort(size)[::-1][:n].sum()) and res.stats[[0, 1, 5, 8, 9]].tolist() == [1, n, short, 3000 - n, 1 - short]
    want = rows.copy()
    r = np.arange(n)
    want[2999 - r, 0] = 7999 - r
    assert (res.rows == want).all()


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------
def test_edge_cases(call):
    res = call(np.zeros((0, 3)), 4, [0, 1, 0, 1], 2, np.zeros(0, dtype=np.int64), max_bytes=100)   # no partition
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0, 0) and res.stats[[0, 1, 2, 4, 5, 6, 7, 8, 9]].tolist() == [0] * 9
    res, _ = _checked(call, dict(rows=np.zeros((5, 1)), size=[3, 0, 4, 1, 9], B=1, rack_of=[0], R=1), 100)   # one broker
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 17, 17, 17) and res.stats[8:].tolist() == [0, 0]
    rng = np.random.default_rng(8)
    c = dict(rows=dr.skewed_rows(rng, 20, 50, 8, pad=0.6), size=rng.integers(1, 1000, 50), B=20, rack_of=np.arange(20) % 4, R=4)
    res, _ = _checked(call, dict(c, size=np.zeros(50, dtype=np.int64)), 0)   # nothing weighs anything
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0, 0) and res.stats[0] == 0 and res.stats[9] == 0
    size = np.where(np.arange(50) % 7 == 0, 0, c["size"] + 10)
    res, ref = _checked(call, dict(c, size=size), 10)   # below the smallest positive size
    assert res.n_moved == 0 and res.stats[0] == 0 and res.stats[9] == int(ref["budget_bound"]) == 1
    res, _ = _checked(call, c, 2 ** 64 - 2)
    free, _ = _checked(call, c, None)
    assert res.n_moved > 0 and res.rows.tobytes() == free.rows.tobytes() and res.stats[[0, 1, 2, 8, 9]].tolist() == free.stats[[0, 1, 2, 8, 9]].tolist()


# ---- 7. the command-line tools -------------------------------------------------------------------------------------------------------
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


def test_cli_end_to_end(kao, tmp_path):
    """cli/kao-disk and the Python twin with --max-bytes on a three-topic document of mixed RF whose replicas crowd a third of the
    brokers: the same bytes, the library's plan, the report's tail; kao-waves takes the plan; without the flag the report is the
    unbudgeted one."""
    from kafka_assignment_optimizer_amd.disk import balance_disk, report_lines
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
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path), "--sizes", str(sizes_path),
            "--default-size", "70K"]
    for prog in PROGS:   # usage errors exit with 2
        for bad in (["--max-bytes", "1X"], ["--max-bytes", "-1"], ["--max-bytes"]):
            assert subprocess.run(prog + base + ["--out", str(tmp_path / "x.json")] + bad, capture_output=True, cwd=ROOT).returncode == 2, bad
    kw = dict(broker_list=ids, racks=racks, default_size=70 * 1024)
    free = balance_disk(doc, sizes_path.read_text(), **kw)
    plan, report = _both(base, tmp_path, "free")   # without the flag: the unbudgeted line, byte for byte
    assert plan == free.document and [report] == report_lines(free) and " max_bytes=" not in report and report.endswith(f" launches={free.result.stats[3]}")
    plan, report = _both(base + ["--max-bytes", "300K"], tmp_path, "cap")
    lib = balance_disk(doc, sizes_path.read_text(), max_bytes=300 * 1024, **kw)
    res = lib.result
    assert plan == lib.document and len(plan["partitions"]) == res.stats[4] and [report] == report_lines(lib)
    assert report.startswith(f"disk: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} lower_bound={res.lower_bound} ")
    assert report.endswith(f" launches={res.stats[3]} max_bytes={300 * 1024} bytes_left={300 * 1024 - res.bytes_moved} refused={res.stats[8]} "
                           f"budget_bound={res.stats[9]}")
    assert 0 < res.bytes_moved <= 300 * 1024 < free.result.bytes_moved and res.stats[9] == 1 and res.peak_after < res.peak_before
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", str(cur_path), "--plan", str(tmp_path / "cap0.json"), "--sizes", str(sizes_path),
                        "--default-size", "70K", "--max-bytes-per-broker", "1M", "--out-prefix", str(tmp_path / "wave")], capture_output=True, cwd=ROOT)
    assert r.returncode == 0 and (tmp_path / "wave1.json").exists(), r.stderr


# ---- 8. the ends of a batch of rounds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_bytes,max_rounds,rounds,stopped", [(3 * 10 ** 8, 0, 87, 0), (3 * 10 ** 8, 32, 32, 1), (3 * 10 ** 8, 64, 64, 1), (3 * 10 ** 8, 87, 87, 0),
                                                                 (3 * 10 ** 8, 88, 87, 0), (10 ** 8, 0, 23, 0)])
def test_budget_ends_and_max_rounds_on_batch_boundaries(call, max_bytes, max_rounds, rounds, stopped):
    """lognormal_case(24, 4, 400, 3, 0.7, 11), one replica per rack: a budget of 3e8 bytes ends the descent after 87 rounds with 3
    winners refused, one of 1e8 after 23.  max_rounds on the end of a batch of 32 rounds, on the last round (the probe finds nothing
    affordable, so the call was not stopped, and the unbudgeted probe follows) and past it.  stats[3] is the launch schedule of
    tests/disk_launches.py."""
    res, ref = _checked(call, dr.lognormal_case(24, 4, 400, 3, 0.7, 11), max_bytes, cap=1, max_rounds=max_rounds)
    assert (ref["rounds"], int(ref["more"])) == (rounds, stopped)
    if not stopped:
        assert (ref["refused"], int(ref["budget_bound"])) == (3, 1)
    assert res.stats[3] == disk_launches(rounds, max_rounds, bool(stopped), budget=True)
