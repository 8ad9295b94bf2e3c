"""kao_place_logdirs on the MI355X: log dirs for the replicas a plan brings to a broker and for those of an evacuated dir, the largest
first onto the lightest dir, one workgroup per broker.  Every instance is held byte for byte (dir[], every
number, per_broker, stats except the launches) against the restatement in tests/place_ref.py; each runs twice for determinism and
once with dry_run, and is checked without the restatement: the bound from the input, the peaks from recomputed loads, no replica
off its broker, every homeless replica placed."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import logdirs_ref as lr
import place_ref as pr
from conftest import ROOT

pytestmark = pytest.mark.gpu

CUTOFF = 4096   # kLdSortLds of kao_logdirs.hip: the most homeless replicas of one broker that the LDS sort takes


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def call(kao):
    from kafka_assignment_optimizer_amd.logdirs import place_logdirs_arrays
    return place_logdirs_arrays


@contextlib.contextmanager
def sort_path(path):
    """The sort of this thread's calls (kao_logdirs_test_sort), put back on the way out."""
    from kafka_assignment_optimizer_amd import _ffi
    was = _ffi.load().kao_logdirs_test_sort(path)
    assert was >= 0
    try:
        yield
    finally:
        _ffi.load().kao_logdirs_test_sort(was)


def _numbers(res):
    return res.status, res.n_placed, res.bytes_placed, res.n_moved, res.bytes_moved, res.peak_before, res.peak_after


def _same(x, y):
    return x.dir.tobytes() == y.dir.tobytes() and _numbers(x) == _numbers(y) and x.per_broker.tobytes() == y.per_broker.tobytes() and x.stats.tolist() == y.stats.tolist()


def _checked(call, c, move=False, min_gain=0, max_rounds=0, paths=False):
    """One instance through the GPU against the restatement; twice, and once with dry_run; every invariant.  paths: through both
    sorts as well.  Returns (result, restatement)."""
    ds, br, d, w, bs = (c["dir_start"], np.asarray(c["broker"], dtype=np.int64), np.asarray(c["dir"], dtype=np.int64), np.asarray(c["size"], dtype=np.int64),
                        c.get("base"))
    args = (ds, br, d, w, bs, move, min_gain, max_rounds)
    ref = pr.place(*args)
    res, again = (call(*args) for _ in range(2))
    dry = call(*args, dry_run=True)
    print(f"B={len(ds) - 1} D={int(np.asarray(ds)[-1])} R={len(d)} move={move} gpu={_numbers(res)} stats={res.stats.tolist()} ref={ref['stats']}")
    assert res.dir.astype(np.int64).tobytes() == ref["dir"].tobytes()
    assert _numbers(res) == (ref["status"], ref["n_placed"], ref["bytes_placed"], ref["n_moved"], ref["bytes_moved"], ref["peak_before"], ref["peak_after"])
    assert [[int(x) for x in row] for row in res.per_broker] == ref["per_broker"]
    assert res.stats[:5].tolist() == ref["stats"][:5] and res.stats[6:].tolist() == ref["stats"][6:] and res.stats[5] in (2, 4)
    # without the restatement
    out, home = res.dir.astype(np.int64), d < 0
    assert (out >= 0).all() and (res.n_placed, res.bytes_placed) == (int(home.sum()), int(w[home].sum()))                     # every homeless replica placed
    assert (lr.broker_of_dir(ds)[out] == br).all() if len(d) else True                                                       # no replica off its broker
    assert res.per_broker[:, 2].tolist() == pr.lower_bound(ds, br, d, w, bs, move)                                           # from the input
    L0, L1 = lr.loads(ds, d[~home], w[~home], bs), lr.loads(ds, out, w, bs)
    assert res.peak_before == int(L0.max(initial=0)) and res.peak_after == int(L1.max(initial=0)) and int(L0.sum()) + int(w[home].sum()) == int(L1.sum())
    assert (res.per_broker[:, 2] <= res.per_broker[:, 1]).all()
    moved = ~home & (out != d)
    assert (res.n_moved, res.bytes_moved) == (int(moved.sum()), int(w[moved].sum())) and (move or not moved.any())
    assert res.status == ("OPTIMAL_PROVEN" if (res.per_broker[:, 1] == res.per_broker[:, 2]).all() else "FEASIBLE_BOUND_GAP")
    if not move:
        assert pr.placed_stable(ds, d, out, w, bs) if len(d) <= 3000 else True
    elif res.stats[6] == 0:
        assert lr.stable(ds, out, w, bs, min_gain)
    assert _same(res, again)
    assert _numbers(dry) == _numbers(res) and (dry.dir == d).all() and dry.per_broker.tobytes() == res.per_broker.tobytes() and dry.stats.tolist() == res.stats.tolist()
    if paths:
        got = []
        for path in (1, 2):
            with sort_path(path):
                got.append(call(*args))
        assert _same(got[0], res) and _same(got[1], res)
    return res, ref


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", [False, True])
def test_small_family_matches_the_restatement(call, move):
    placed = proven = 0
    for seed in range(120):
        res, _ = _checked(call, pr.small_case(seed), move, paths=seed % 4 == 0)
        placed += res.n_placed > 0
        proven += res.status == "OPTIMAL_PROVEN"
    print(f"calls with a homeless replica: {placed} of 120, proven optimal: {proven}")
    assert placed >= 90 and (move or proven >= 85)   # (the bound over base alone, with move_residents, proves fewer)


# ---- 2. homeless counts ----------------------------------------------------------------------------------------------------------------
def _one_big(k, n, residents, seed, sizes=None):
    """Broker 1 has n dirs, `residents` residents and k homeless replicas; three small brokers around it; the array order is shuffled."""
    big = lr.lognormal_case(1, n, residents + k, 0.7, seed)
    rng = np.random.default_rng(seed)
    bd = big["dir"].copy()
    bd[rng.permutation(residents + k)[:k]] = -1
    bw = big["size"] if sizes is None else sizes
    ds = np.array([0, 2, 2 + n, 4 + n, 6 + n])
    d = np.concatenate([[0, -1], np.where(bd >= 0, bd + 2, -1), [2 + n, -1, 5 + n]])
    broker = np.concatenate([[0, 0], np.ones(residents + k, dtype=np.int64), [2, 2, 3]])
    size = np.concatenate([[700, 30], bw, [0, 55, 900]])
    perm = rng.permutation(len(d))
    return dict(dir_start=ds, broker=broker[perm], dir=d[perm], size=size[perm], base=None)


@pytest.mark.parametrize("move", [False, True])
@pytest.mark.parametrize("k", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, CUTOFF - 1, CUTOFF, CUTOFF + 1, 2500])
def test_homeless_counts(kao, call, k, move):
    """One broker with k homeless replicas and 40 residents among three small ones: a list below, at and above a chunk of the greedy
    pass, a power of two and its neighbours (2,500 is none: the padding), and the two sides of the cut-off between the sorts.  Both
    sorts are forced wherever both can run; the LDS sort refuses a count above the cut-off."""
    n = 12 if k == 2500 else 4
    c = _one_big(k, n, 40, 100 + k)
    res, ref = _checked(call, c, move, paths=k <= CUTOFF)
    assert res.per_broker[1, 3] == k and res.stats[9] == max(k, 1) and res.per_broker[[0, 2, 3], 3].tolist() == [1, 1, 0]
    if k >= 63 and not move:   # largest first onto the lightest dir levels a skewed broker
        assert res.per_broker[1, 1] == res.per_broker[1, 2] or res.per_broker[1, 1] - res.per_broker[1, 2] <= c["size"].max()
    if k > CUTOFF:
        with sort_path(1):
            with pytest.raises(kao.KaoError) as e:
                call(c["dir_start"], c["broker"], c["dir"], c["size"], None, move)
            assert e.value.code == -2 and "homeless" in str(e.value)
        with sort_path(2):
            assert _same(call(c["dir_start"], c["broker"], c["dir"], c["size"], None, move), res)


# ---- 3. ties, wide loads, zero sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", [False, True])
def test_ties(call, move):
    for k in (7, 64, 300):
        c = _one_big(k, 4, 0, k, sizes=np.full(k, 5, dtype=np.int64))   # all sizes equal, all dirs empty: r alone orders, the lowest dir wins
        res, _ = _checked(call, c, move, paths=True)
        mine = np.nonzero(c["broker"] == 1)[0]                          # ascending r: dirs 0, 1, 2, 3, 0, 1, ..
        assert (res.dir[mine] == 2 + np.arange(k) % 4).all() and res.n_moved == 0
        c = _one_big(k, 4, 40, k, sizes=np.full(40 + k, 5, dtype=np.int64))
        _checked(call, c, move, paths=True)


@pytest.mark.parametrize("move", [False, True])
def test_loads_pass_2_32_and_2_48(call, move):
    """Sizes of 2^40 + a little: the loads pass 2^32 and 2^48, so the argmin compares both halves of a load."""
    k = 1500
    c = _one_big(k, 4, 40, 5, sizes=2 ** 40 + (np.arange(40 + k) * 7919) % 13)
    res, _ = _checked(call, c, move, paths=True)
    assert res.peak_after > 2 ** 48 and res.per_broker[1, 1] - res.per_broker[1, 2] <= 2 ** 40 + 13
    c = _one_big(k, 4, 40, 6, sizes=np.where(np.arange(40 + k) % 2 == 0, 2 ** 33, 3).astype(np.int64))   # loads that differ in one half only
    _checked(call, c, move, paths=True)


@pytest.mark.parametrize("move", [False, True])
def test_a_tenth_of_the_sizes_zero(call, move):
    c = _one_big(400, 4, 40, 8)   # the log-normal family has a tenth of its sizes at zero
    assert 20 <= (c["size"] == 0).sum() <= 80
    res, _ = _checked(call, c, move, paths=True)
    c = _one_big(70, 4, 0, 9, sizes=np.zeros(70, dtype=np.int64))   # nothing but zeros
    res, _ = _checked(call, c, move, paths=True)
    assert res.per_broker[1].tolist()[:5] == [0, 0, 0, 70, 0] and (res.dir[c["broker"] == 1] == 2).all()   # dir 0 of the broker stays the lightest


# ---- 4. dir counts, empty brokers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", [False, True])
@pytest.mark.parametrize("n", [1, 2, 64])
def test_dir_counts(call, n, move):
    res, _ = _checked(call, _one_big(200, n, 60, n), move, paths=True)
    assert res.per_broker[1, 3] == 200
    if n == 1:
        assert res.per_broker[1, 1] == res.per_broker[1, 2] and res.n_moved == 0


@pytest.mark.parametrize("move", [False, True])
def test_empty_brokers(call, move):
    rng = np.random.default_rng(3)
    w = rng.integers(1, 1000, 90).astype(np.int64)
    # broker 0: neither dirs nor replicas; broker 1: 6 empty dirs that receive everything (the expansion); broker 2: dirs and bases, no replica
    c = dict(dir_start=[0, 0, 6, 9], broker=np.ones(90, dtype=np.int64), dir=np.full(90, -1), size=w, base=[0, 0, 0, 0, 0, 0, 4, 0, 9])
    res, _ = _checked(call, c, move, paths=True)
    assert res.per_broker[0].tolist() == [0] * 8 and res.per_broker[2].tolist() == [9, 9, 9, 0, 0, 0, 0, 0]
    assert res.per_broker[1, 0] == 0 and res.per_broker[1, 3] == 90 and res.peak_before == 9 and res.n_moved == 0
    assert res.per_broker[1, 1] - res.per_broker[1, 2] < 1000
    res, _ = _checked(call, dict(dir_start=[0, 0, 0], broker=np.zeros(0, dtype=np.int64), dir=np.zeros(0, dtype=np.int64), size=np.zeros(0, dtype=np.int64)), move)
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0, 0, 0) and res.stats[7] == 2 and res.stats[5] == 2


# ---- 5. residents only: the two identities ---------------------------------------------------------------------------------------------
def test_residents_only(call):
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays
    for c in [lr.small_case(s) for s in range(0, 120, 7)] + [lr.lognormal_case(5, 6, 300, 1.0, 4, based=1 / 3), lr.lognormal_case(1, 12, 2500, 0.7, 5)]:
        broker = lr.broker_of_dir(c["dir_start"])[c["dir"]] if len(c["dir"]) else np.zeros(0, dtype=np.int64)
        pc = dict(c, broker=broker)
        for kw in (dict(), dict(min_gain=9), dict(max_rounds=2)):
            want = balance_logdirs_arrays(c["dir_start"], c["dir"], c["size"], c["base"], **kw)
            res, _ = _checked(call, pc, True, kw.get("min_gain", 0), kw.get("max_rounds", 0))
            assert res.dir.tobytes() == want.dir.tobytes() and res.n_placed == 0 and res.status == want.status
            assert (res.n_moved, res.bytes_moved, res.peak_before, res.peak_after) == (want.n_moved, want.bytes_moved, want.peak_before, want.peak_after)
            assert res.per_broker[:, [0, 1, 2, 5, 6, 7]].tobytes() == want.per_broker.tobytes() and (res.per_broker[:, [3, 4]] == 0).all()
            assert res.stats[[1, 2, 3, 4, 6, 7, 8]].tolist() == want.stats[[0, 1, 2, 3, 5, 6, 7]].tolist()
        res, _ = _checked(call, pc, False)   # the residents stay: nothing changes, every broker is proven
        assert (res.dir == c["dir"]).all() and res.status == "OPTIMAL_PROVEN" and res.peak_after == res.peak_before and res.stats[7] == len(c["dir_start"]) - 1


# ---- 6. many brokers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", [False, True])
def test_many_brokers_are_independent(call, move):
    """300 brokers x 4 dirs x (20 residents + 20 homeless) in one call: the row of every broker is what the restatement gives on that
    broker alone (its replicas keep the r of the call's arrays)."""
    c = lr.lognormal_case(300, 4, 40, 0.7, 9, based=1 / 3)
    broker, d = c["dir"] // 4, c["dir"].copy()
    rng = np.random.default_rng(11)
    for b in range(300):
        d[rng.permutation(np.nonzero(broker == b)[0])[:20]] = -1
    c = dict(c, broker=broker, dir=d)
    res, ref = _checked(call, c, move)
    assert res.stats[0] == 300 and res.n_placed == 6000 and (res.per_broker[:, 3] == 20).all() and (not move or res.stats[1] > 0)
    for b in range(300):
        one, mine = pr.one_broker(c, b)
        alone = pr.place(**one, move_residents=move, ids=mine)
        assert alone["per_broker"][0] == [int(x) for x in res.per_broker[b]]
        assert (alone["dir"] + 4 * b == res.dir[mine]).all()


def test_invalid_arguments_leave_dir_alone(kao):
    """Every refusal of include/kao.h is one on a machine with a device too."""
    import test_place_errors as host
    for what, change, code, text in host.REFUSED:
        for move in (0, 1):
            rc, msg = host._call(move_residents=move, **change)
            assert rc == code and text in msg, what


# ---- 7. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-logdirs")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.logdirs"])


def _both(args, tmp_path, tag):
    """Each tool in a fresh child process: the same --out document and the same report."""
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"{tag}{i}.json"
        r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    return outs[0][0], outs[0][1].splitlines()


def test_cli_against_python(kao, tmp_path):
    """cli/kao-logdirs and the Python twin with --plan, --evacuate and --rebalance on a generated cluster of 9 brokers with two to four
    dirs each, the plan moving about a quarter of the replicas to other brokers: the same plan file, the same report, both the
    library's; and without the new flags what the tool wrote before them."""
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs, place_logdirs
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(7)
    ids = [100 + 3 * i for i in range(9)]
    ndirs = {b: int(rng.integers(2, 5)) for b in ids}
    doc, held = {"version": 1, "partitions": []}, {b: [[] for _ in range(ndirs[b])] for b in ids}
    plan = {"version": 1, "partitions": []}
    for name, P, rf in (("alpha", 30, 3), ("be-ta", 20, 2), ("gamma", 12, 1)):
        for p in range(P):
            r = rng.permutation(9)[:rf]
            row = [ids[b] for b in r]
            doc["partitions"].append({"topic": name, "partition": p, "replicas": row})
            w = int(rng.integers(1, 1000))
            for b in r:   # most replicas land in the first dir
                i = 0 if rng.random() < 0.7 else int(rng.integers(0, ndirs[ids[b]]))
                held[ids[b]][i].append({"partition": f"{name}-{p}", "size": w * 1024 - int(b), "offsetLag": 0, "isFuture": False})
            new = list(row)
            for j in range(rf):   # about a quarter of the replicas go to a broker outside the row
                if rng.random() < 0.25:
                    new[j] = int(rng.choice([b for b in ids if b not in new and b not in row]))
            if new != row:
                plan["partitions"].append({"topic": name, "partition": p, "replicas": new})
    doc["partitions"].append({"topic": "gamma", "partition": 99, "replicas": [ids[0]]})                  # no entry anywhere: no size
    held[ids[0]][1].append({"partition": "alpha-0", "size": 77777, "offsetLag": 5, "isFuture": True})    # a future copy: base
    held[ids[1]][0].append({"partition": "dropped-4", "size": 55555, "offsetLag": 0, "isFuture": False})  # not in --current: base
    logdirs = {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": f"/data/d{ndirs[b] - i}", "error": None, "partitions": e} for i, e in enumerate(held[b])]
                                          + ([{"logDir": "/data/broken", "error": "KafkaStorageException", "partitions": []}] if b == ids[2] else [])} for b in ids]}
    nosize = {"version": 1, "partitions": plan["partitions"] + [{"topic": "gamma", "partition": 99, "replicas": [ids[1]]}]}
    cur_path, dirs_path, plan_path, nosize_path = (tmp_path / n for n in ("current.json", "logdirs.txt", "plan.json", "nosize.json"))
    cur_path.write_text(json.dumps(doc))
    plan_path.write_text(json.dumps(plan))
    nosize_path.write_text(json.dumps(nosize))
    text_in = "Querying brokers for log directories information\nReceived log directory information from brokers\n" + json.dumps(logdirs) + "\n"
    dirs_path.write_text(text_in)
    cur = {(e["topic"], e["partition"]): e["replicas"] for e in doc["partitions"]}
    tgt = {(e["topic"], e["partition"]): e["replicas"] for e in plan["partitions"]}
    n_arrivals = sum(b not in cur[k] for k, row in tgt.items() for b in row)
    assert 25 <= n_arrivals <= 45 and 30 <= len(tgt) < 62   # about a quarter of 142 replicas; the plan is a subset
    base = ["--current", str(cur_path), "--log-dirs", str(dirs_path)]
    x = str(tmp_path / "x.json")
    bad1, bad2 = tmp_path / "bad1.json", tmp_path / "bad2.json"
    bad1.write_text(json.dumps({"version": 1, "partitions": [{"topic": "alpha", "partition": 777, "replicas": [ids[0]]}]}))
    bad2.write_text(json.dumps({"version": 1, "partitions": [{"topic": "alpha", "partition": 0, "replicas": [ids[0], ids[1], ids[0]]}]}))
    for prog in PROGS:   # usage errors exit with 2, input errors with 1
        for bad in (["--rebalance"], ["--default-size", "1K"], ["--plan", str(plan_path), "--default-size", "1X"], ["--evacuate", "nodir"], ["--evacuate", f"{ids[0]}:"],
                    ["--evacuate", ":/data/d1"], ["--plan"]):
            assert subprocess.run(prog + base + ["--out", x] + bad, capture_output=True, cwd=ROOT).returncode == 2, bad
        for bad in (["--plan", str(bad1)], ["--plan", str(bad2)], ["--evacuate", f"{ids[0]}:/data/nosuch"], ["--evacuate", "999:/data/d1"], ["--evacuate", f"{ids[2]}:/data/broken"],
                    ["--evacuate", f"{ids[0]}:/data/d1", "--broker-list", str(ids[1])], ["--plan", str(nosize_path)],
                    [a for i in range(ndirs[ids[0]]) for a in ("--evacuate", f"{ids[0]}:/data/d{i + 1}")]):
            r = subprocess.run(prog + base + ["--out", x] + bad, capture_output=True, cwd=ROOT)
            assert r.returncode == 1 and b"kao-logdirs: " in r.stderr, (bad, r.stderr)
    # the new flags
    ev = [(ids[3], "/data/d1"), (ids[5], "/data/d2")]
    evf = [a for b, n in ev for a in ("--evacuate", f"{b}:{n}")]
    some = [ids[4], ids[0], ids[3], 999]
    for tag, flags, kw in (("plan", ["--plan", str(plan_path)], dict(plan_doc=plan)),
                           ("rebal", ["--plan", str(plan_path), "--rebalance", "--min-gain", "16K"], dict(plan_doc=plan, rebalance=True, min_gain=16384)),
                           ("evac", evf, dict(evacuate=ev)),
                           ("both", ["--plan", str(plan_path), "--rebalance"] + evf, dict(plan_doc=plan, rebalance=True, evacuate=ev)),
                           ("dry", ["--plan", str(plan_path), "--dry-run"] + evf, dict(plan_doc=plan, evacuate=ev, dry_run=True)),
                           ("nosize", ["--plan", str(nosize_path), "--default-size", "5K"], dict(plan_doc=nosize, default_size=5120)),
                           ("some", ["--plan", str(plan_path), "--broker-list", ",".join(str(b) for b in some)] + evf[:2], dict(plan_doc=plan, broker_list=some, evacuate=ev[:1]))):
        text, report = _both(base + flags, tmp_path, tag)
        lib = place_logdirs(doc, text_in, **kw)
        res, out = lib.result, json.loads(text)
        assert text.decode() == lib.text() and out == lib.document() and report == lib.report_lines()
        listed = some[:3] if tag == "some" else ids
        assert len(report) == len(kw.get("broker_list", ids)) + 1 and report[-1].startswith(f"logdirs: status={res.status} brokers={len(report) - 1} ")
        assert f" replicas_placed={res.n_placed} bytes_placed={res.bytes_placed} replicas_moved={res.n_moved} bytes_moved={res.bytes_moved} " in report[-1]
        assert f" evacuated_dirs={len(kw.get('evacuate', ()))} " in report[-1] and " stranded_bytes=" in report[-1] and f" homeless={res.n_placed} " in report[-1]
        assert res.n_placed > 0 and (res.n_moved > 0) == ("rebalance" in kw)
        if tag == "dry":
            assert out["partitions"] == []
            continue
        want = nosize if tag == "nosize" else plan if "plan_doc" in kw else {"partitions": []}
        rows = {(e["topic"], e["partition"]): e["replicas"] for e in want["partitions"]}
        seen, named = set(), 0
        for e in out["partitions"]:
            k = (e["topic"], e["partition"])
            seen.add(k)
            assert e["replicas"] == rows.get(k, cur[k]) and len(e["log_dirs"]) == len(e["replicas"])
            assert k in rows or any(n != "any" for n in e["log_dirs"])
            for b, n in zip(e["replicas"], e["log_dirs"]):
                assert n == "any" or (n.startswith("/data/d") and b in listed and (b, n) not in kw.get("evacuate", ()))   # no evacuated dir is a destination
                if b not in cur[k]:
                    assert (n != "any") == (b in listed)   # every arrival on a listed broker has a dir by name
                named += n != "any"
        assert set(rows) <= seen and named == res.n_placed + res.n_moved   # every slot that is neither placed nor moved says "any"
        assert [(e["topic"].encode(), e["partition"]) for e in out["partitions"]] == sorted((e["topic"].encode(), e["partition"]) for e in out["partitions"])
        if tag == "nosize":
            assert {"topic": "gamma", "partition": 99, "replicas": [ids[1]]}.items() <= [e for e in out["partitions"] if e["partition"] == 99][0].items()
        if tag == "evac":   # every non-future entry of the two dirs whose partition is in --current is rescued; nothing else is in the plan
            gone = sum(not e["isFuture"] and tuple(e["partition"].rsplit("-", 1)) in {(t, str(p)) for t, p in cur}
                       for b, n in ev for e in held[b][ndirs[b] - int(n[-1])])
            assert res.n_placed == gone > 0 and " stranded_bytes=0 " in report[-1]
    # without the new flags: the tool as it was
    for tag, flags, kw in (("old", [], {}), ("oldgain", ["--min-gain", "64K"], dict(min_gain=65536))):
        text, report = _both(base + flags, tmp_path, tag)
        lib = balance_logdirs(doc, text_in, **kw)
        assert text.decode() == lib.text() and report == lib.report_lines() and lib.result.n_moved > 0
