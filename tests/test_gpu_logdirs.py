"""kao_balance_logdirs on the MI355X: replica moves between the log dirs of one broker that lower the peak of the bytes a dir stores,
one workgroup per broker, every broker in one launch.  Every instance is held byte for byte (dir[], every
number, per_broker, stats[0..3] and [5..7]) against the restatement of the rounds in tests/logdirs_ref.py; each runs twice for
determinism and once with dry_run, and is checked for the invariants without the restatement: move-stable unless stopped, and the
bound recomputed from the input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import logdirs_ref as lr
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def call(kao):
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays
    return balance_logdirs_arrays


def _numbers(res):
    return res.status, res.n_moved, res.bytes_moved, res.peak_before, res.peak_after


def _same(x, y):
    return x.dir.tobytes() == y.dir.tobytes() and _numbers(x) == _numbers(y) and x.per_broker.tobytes() == y.per_broker.tobytes()


def _checked(call, c, min_gain=0, max_rounds=0):
    """One instance through the GPU against the restatement; twice, and once with dry_run; every invariant.  Returns (result, restatement)."""
    ds, d, w, bs = c["dir_start"], np.asarray(c["dir"], dtype=np.int64), np.asarray(c["size"], dtype=np.int64), c.get("base")
    ref = lr.descend(ds, d, w, bs, min_gain, max_rounds)
    res, again = (call(ds, d, w, bs, min_gain, max_rounds) for _ in range(2))
    dry = call(ds, d, w, bs, min_gain, max_rounds, dry_run=True)
    print(f"B={len(ds) - 1} D={int(ds[-1])} R={len(d)} gpu={_numbers(res)} stats={res.stats.tolist()} ref={ref['stats']}")
    assert res.dir.astype(np.int64).tobytes() == ref["dir"].tobytes()
    assert _numbers(res) == (ref["status"], ref["n_moved"], ref["bytes_moved"], ref["peak_before"], ref["peak_after"])
    assert [[int(x) for x in row] for row in res.per_broker] == ref["per_broker"]
    assert res.stats[:4].tolist() == ref["stats"][:4] and res.stats[5:].tolist() == ref["stats"][5:] and res.stats[4] in (2, 4)
    # without the restatement
    out = res.dir.astype(np.int64)
    assert res.per_broker[:, 2].tolist() == lr.lower_bound(ds, d, w, bs)   # from the input
    L0, L1 = lr.loads(ds, d, w, bs), lr.loads(ds, out, w, bs)
    assert res.peak_before == int(L0.max(initial=0)) and res.peak_after == int(L1.max(initial=0)) and int(L0.sum()) == int(L1.sum())
    assert (res.per_broker[:, 2] <= res.per_broker[:, 1]).all() and (res.per_broker[:, 1] <= res.per_broker[:, 0]).all()
    assert (lr.broker_of_dir(ds)[out] == lr.broker_of_dir(ds)[d]).all() if len(d) else True   # no replica leaves its broker
    assert (res.n_moved, res.bytes_moved) == (int((out != d).sum()), int(w[out != d].sum()))
    assert res.status == ("OPTIMAL_PROVEN" if (res.per_broker[:, 1] == res.per_broker[:, 2]).all() else "FEASIBLE_BOUND_GAP")
    if res.stats[5] == 0:
        assert lr.stable(ds, out, w, bs, min_gain)
    assert _same(res, again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.dir == d).all() and dry.per_broker.tobytes() == res.per_broker.tobytes() and dry.stats.tolist() == res.stats.tolist()
    return res, ref


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_matches_the_restatement(call):
    proven = moved = 0
    for seed in range(120):
        res, _ = _checked(call, lr.small_case(seed))
        proven += res.status == "OPTIMAL_PROVEN"
        moved += res.n_moved > 0
    print(f"proven optimal: {proven} of 120, moved: {moved}")
    assert moved >= 60 and 10 <= proven <= 110


# ---- 2. dir counts -------------------------------------------------------------------------------------------------------------------
def _mixed(nd, per_dir, seed):
    """Brokers with nd[b] dirs, about per_dir replicas a dir placed with a skew toward the low dirs, a third of the dirs with a base."""
    rng = np.random.default_rng(seed)
    ds = np.concatenate([[0], np.cumsum(nd)]).astype(np.int64)
    d = np.concatenate([ds[b] + lr._skewed_dirs(rng, n, per_dir * n) for b, n in enumerate(nd) if n] or [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    rng.shuffle(d)
    D = int(ds[-1])
    return dict(dir_start=ds, dir=d, size=rng.integers(0, 1000, len(d)).astype(np.int64), base=np.where(rng.random(D) < 1 / 3, rng.integers(1, 3000, D), 0))


def test_dir_count_edges(call):
    res, _ = _checked(call, _mixed([0, 1, 2, 63, 64, 0, 3], 3, 1))   # 0, 1, 2, 63 and KAO_LOGDIRS_MAX_DIRS dirs in one call
    assert res.per_broker[0].tolist() == [0] * 6 and res.per_broker[1, 3] == 0 and (res.per_broker[[2, 3, 4], 3] > 0).all()
    res, _ = _checked(call, _mixed([5], 4, 2))                       # one broker
    assert res.n_moved > 0 and res.stats[0] == 1
    c = _mixed([3, 4], 3, 3)
    keep = c["dir"] >= 3                                            # broker 0 keeps its dirs and bases, and loses its replicas
    c = dict(c, dir=c["dir"][keep], size=c["size"][keep], base=np.array([5, 0, 9, 0, 0, 0, 0]))
    res, _ = _checked(call, c)
    assert res.per_broker[0].tolist() == [9, 9, 9, 0, 0, 0] and res.per_broker[1, 3] > 0
    res, _ = _checked(call, dict(dir_start=[0, 2, 2, 5], dir=np.zeros(0, dtype=np.int64), size=np.zeros(0, dtype=np.int64), base=[1, 2, 0, 0, 7]))   # no replica
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 7, 7) and res.stats[4] == 2 and res.per_broker[:, 2].tolist() == [2, 0, 7]
    res, _ = _checked(call, dict(dir_start=[0, 0, 0], dir=np.zeros(0, dtype=np.int64), size=np.zeros(0, dtype=np.int64)))   # no dir either
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 0) and res.stats[6] == 2
    res, _ = _checked(call, dict(_mixed([4, 6], 5, 4), base=None))   # base == NULL
    assert res.n_moved > 0


# ---- 3. bucket sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 2500])
def test_bucket_sizes(call, k):
    """One broker holds k replicas, three others one each: a bucket below, at and above a wavefront and a 256-lane workgroup; 1,024 is
    the last size the 256-lane workgroup takes and 1,025 the first of the 1,024-lane one; 2,500 on 12 dirs makes 1,024 lanes stride."""
    n = 12 if k == 2500 else 4
    big = lr.lognormal_case(1, n, k, 0.7, k)
    ds = np.array([0, 2, 2 + n, 4 + n, 6 + n])
    d = np.concatenate([[0], big["dir"] + 2, [2 + n, 5 + n]])
    size = np.concatenate([[700], big["size"], [0, 900]])
    perm = np.random.default_rng(k).permutation(len(d))
    res, ref = _checked(call, dict(dir_start=ds, dir=d[perm], size=size[perm], base=None))
    assert res.per_broker[[0, 2, 3], 3].tolist() == [0, 0, 0] and (k < 63 or res.per_broker[1, 3] > 0)
    assert k < 63 or res.per_broker[1, 1] < res.per_broker[1, 0]


# ---- 4. contention -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dirs", [2, 3, 64])
def test_every_replica_on_one_dir(call, n_dirs):
    """Every replica on dir 0: one source, so one move a round.  Equal sizes: every key ties down to r.  Sizes of 2^40 + a little: the
    loads pass 2^32 and 2^48."""
    for n in (64, 257, 1500):
        for base in (0, 2 ** 40):
            res, ref = _checked(call, lr.crowded_case(n_dirs, n, base=base))
            assert res.n_moved > 0 and res.stats[2] >= res.n_moved and res.stats[1] == res.stats[7]
            if base:
                assert res.peak_before > 2 ** 40 * n >= 2 ** 46 and (n < 257 or res.peak_before > 2 ** 48)
            else:   # dir 0 stays the only source: one move a round, none comes back
                assert res.stats[1] == res.stats[2] == res.n_moved
                assert res.peak_after == 5 * -(-n // n_dirs)   # move-stable with equal sizes: no two dirs differ by more than one replica
    c = lr.crowded_case(n_dirs, 257)
    none, _ = _checked(call, c, min_gain=257 * 5)   # no gap is that large
    assert none.n_moved == 0 and none.stats[1] == 0 and none.stats[5] == 0
    huge, _ = _checked(call, c, min_gain=2 ** 64 - 1)
    assert huge.n_moved == 0 and huge.stats[1] == 0
    one, _ = _checked(call, c, max_rounds=1)
    assert one.stats[1] == 1 and one.stats[5] == 1 and one.n_moved == 1 and one.stats[3] == 257


# ---- 5. the bound's terms ------------------------------------------------------------------------------------------------------------
def test_bound_terms_with_bases(call):
    res, _ = _checked(call, dict(dir_start=[0, 3], dir=[0, 0, 1], size=[4, 5, 6], base=[0, 0, 100]))   # (2): a base above everything
    assert res.per_broker[0].tolist()[:3] == [100, 100, 100] and res.status == "OPTIMAL_PROVEN"
    res, _ = _checked(call, dict(dir_start=[0, 3], dir=[0, 0, 0], size=[50, 1, 1], base=[0, 9, 8]))     # (0): 50 + 0 > ceil(69 / 3), 9
    assert res.per_broker[0].tolist()[:4] == [52, 50, 50, 2] and res.status == "OPTIMAL_PROVEN"
    res, _ = _checked(call, dict(dir_start=[0, 3], dir=[0, 0, 0], size=[50, 1, 1], base=[7, 9, 8]))     # (0) again, 50 + 7; the heaviest replica goes first: 58
    assert res.per_broker[0].tolist()[:4] == [59, 58, 57, 1] and res.status == "FEASIBLE_BOUND_GAP"
    res, _ = _checked(call, dict(dir_start=[0, 2], dir=[0, 0, 0], size=[3, 3, 3], base=[0, 1]))         # (1): ceil(10 / 2)
    assert res.per_broker[0].tolist()[:3] == [9, 6, 5] and res.status == "FEASIBLE_BOUND_GAP"


# ---- 6. many brokers -----------------------------------------------------------------------------------------------------------------
def test_many_brokers_are_independent(call):
    """300 brokers x 4 dirs x 40 replicas in one call: the row of per_broker of every broker is what the restatement gives on that
    broker alone (its replicas keep the r of the call's arrays in their keys)."""
    c = lr.lognormal_case(300, 4, 40, 0.7, 9, based=1 / 3)
    res, ref = _checked(call, c)
    assert res.stats[0] > 250 and res.peak_after < res.peak_before
    for b in range(300):
        one, mine = lr.one_broker(c, b)
        alone = lr.descend(**one, ids=mine)
        assert alone["per_broker"][0] == [int(x) for x in res.per_broker[b]]
        assert (alone["dir"] + 4 * b == res.dir[mine]).all()


def test_invalid_arguments_leave_dir_alone(kao):
    """Every refusal of include/kao.h is one on a machine with a device too."""
    import test_logdirs_errors as host
    for what, change, code, text in host.REFUSED:
        rc, msg = host._call(**change)
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
    """cli/kao-logdirs and the Python twin on a generated kafka-log-dirs document with two to four dirs a broker: the same plan file,
    the same report, and both are the library's."""
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(7)
    ids = [100 + 3 * i for i in range(9)]
    ndirs = {b: int(rng.integers(2, 5)) for b in ids}
    doc, held = {"version": 1, "partitions": []}, {b: [[] for _ in range(ndirs[b])] for b in ids}
    for name, P, rf in (("alpha", 30, 3), ("be-ta", 20, 2), ("gamma", 12, 1)):
        for p in range(P):
            r = rng.permutation(9)[:rf]
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
            w = int(rng.integers(1, 1000))
            for b in r:   # most replicas land in the first dir
                i = 0 if rng.random() < 0.7 else int(rng.integers(0, ndirs[ids[b]]))
                held[ids[b]][i].append({"partition": f"{name}-{p}", "size": w * 1024 - int(b), "offsetLag": 0, "isFuture": False})
    held[ids[0]][1].append({"partition": "alpha-0", "size": 77777, "offsetLag": 5, "isFuture": True})    # a future copy: base
    held[ids[1]][0].append({"partition": "dropped-4", "size": 55555, "offsetLag": 0, "isFuture": False})  # not in --current: base
    logdirs = {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": f"/data/d{ndirs[b] - i}", "error": None, "partitions": e} for i, e in enumerate(held[b])]
                                          + ([{"logDir": "/data/broken", "error": "KafkaStorageException", "partitions": []}] if b == ids[2] else [])} for b in ids]}
    cur_path, dirs_path = tmp_path / "current.json", tmp_path / "logdirs.txt"
    cur_path.write_text(json.dumps(doc))
    dirs_path.write_text("Querying brokers for log directories information\nReceived log directory information from brokers\n" + json.dumps(logdirs) + "\n")
    base = ["--current", str(cur_path), "--log-dirs", str(dirs_path)]
    for prog in PROGS:   # usage errors exit with 2, input errors with 1
        assert subprocess.run(prog + base, capture_output=True, cwd=ROOT).returncode == 2   # no --out
        for bad in (["--min-gain", "1X"], ["--max-rounds", "-1"], ["--racks", "x"]):
            assert subprocess.run(prog + base + ["--out", str(tmp_path / "x.json")] + bad, capture_output=True, cwd=ROOT).returncode == 2, bad
        r = subprocess.run(prog + ["--current", str(cur_path), "--log-dirs", str(cur_path), "--out", str(tmp_path / "x.json")], capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"kao-logdirs: " in r.stderr
    some = ",".join(str(b) for b in (ids[4], ids[0], ids[2], 999))
    cur = {(e["topic"], e["partition"]): e["replicas"] for e in doc["partitions"]}
    for tag, flags, kw in (("plain", [], {}), ("gain", ["--min-gain", "64K"], dict(min_gain=65536)), ("one", ["--max-rounds", "1"], dict(max_rounds=1)),
                           ("dry", ["--dry-run"], dict(dry_run=True)), ("some", ["--broker-list", some], dict(broker_list=[ids[4], ids[0], ids[2], 999]))):
        text, report = _both(base + flags, tmp_path, tag)
        lib = balance_logdirs(doc, dirs_path.read_text(), **kw)
        res, plan = lib.result, json.loads(text)
        assert text.decode() == lib.text() and plan == lib.document() and report == lib.report_lines()
        n_brokers = 4 if tag == "some" else 9
        assert len(report) == n_brokers + 1 and report[-1].startswith(f"logdirs: status={res.status} brokers={n_brokers} ")
        assert f" replicas_moved={res.n_moved} bytes_moved={res.bytes_moved} " in report[-1] and f" rounds={res.stats[1]} moves={res.stats[2]} " in report[-1]
        assert res.n_moved > 0 and res.peak_after <= res.peak_before
        moved = 0
        for e in plan["partitions"]:
            assert e["replicas"] == cur[(e["topic"], e["partition"])] and len(e["log_dirs"]) == len(e["replicas"])
            assert any(x != "any" for x in e["log_dirs"]) and all(x == "any" or x.startswith("/data/d") for x in e["log_dirs"])
            moved += sum(x != "any" for x in e["log_dirs"])
        assert moved == (0 if tag == "dry" else res.n_moved)
        if tag == "some":
            assert all(b in (ids[4], ids[0], ids[2]) for e in plan["partitions"] for b, x in zip(e["replicas"], e["log_dirs"]) if x != "any")
            assert " skipped_dirs=1 " in report[-1] and report[3].startswith("logdirs: broker=999 dirs=0 ")
