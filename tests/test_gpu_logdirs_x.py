"""kao_balance_logdirs_exchange on the MI355X: the descent of kao_balance_logdirs with exchange rounds where no move is left, one
workgroup per broker.  Every instance goes through the C ABI and is held bit for bit (dir[], every number,
per_broker, stats except the launches) against the restatement of the rounds in tests/logdirs_x_ref.py, which asserts the
definition's claims every round; each runs once more with dry_run, and its peaks are compared broker by broker with those of
kao_balance_logdirs on the GPU."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import logdirs_ref as lr
import logdirs_x_ref as lx
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def lib(kao):
    from kafka_assignment_optimizer_amd import _ffi
    return _ffi.load()


def _abi(lib, name, c, min_gain=0, max_rounds=0, dry_run=False):
    """One call through the C ABI: (return code, dict of every output as Python ints / arrays)."""
    W, S = (8, 12) if name == "kao_balance_logdirs_exchange" else (6, 8)
    ds = np.ascontiguousarray(c["dir_start"], dtype=np.int32)
    B, R = len(ds) - 1, len(c["dir"])
    d = np.ascontiguousarray(c["dir"], dtype=np.int32) if R else np.zeros(1, dtype=np.int32)
    w = np.ascontiguousarray(c["size"], dtype=np.uint64) if R else np.zeros(1, dtype=np.uint64)
    bs = None if c.get("base") is None else np.concatenate([np.asarray(c["base"], dtype=np.uint64), np.zeros(1, dtype=np.uint64)])   # (never empty)
    n, status = C.c_int32(0), C.c_int32(0)
    moved, before, after = (C.c_uint64(0) for _ in range(3))
    per, stats = np.zeros((B, W), dtype=np.uint64), np.zeros(S, dtype=np.int64)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    rc = getattr(lib, name)(B, ds.ctypes.data_as(i32p), None if bs is None else bs.ctypes.data_as(u64p), R, d.ctypes.data_as(i32p), w.ctypes.data_as(u64p),
                            int(min_gain), int(max_rounds), int(dry_run), C.byref(n), C.byref(moved), C.byref(before), C.byref(after), per.ctypes.data_as(u64p),
                            C.byref(status), stats.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, dict(dir=d[:R].astype(np.int64), n_moved=int(n.value), bytes_moved=int(moved.value), peak_before=int(before.value), peak_after=int(after.value),
                    per_broker=[[int(x) for x in row] for row in per], status={0: "OPTIMAL_PROVEN", 1: "FEASIBLE_BOUND_GAP"}[int(status.value)],
                    stats=[int(x) for x in stats])


NUMBERS = ("n_moved", "bytes_moved", "peak_before", "peak_after", "per_broker", "status")


def _checked(lib, c, min_gain=0, max_rounds=0, ref=None):
    """One instance through the GPU against the restatement, and once with dry_run; its peaks beside kao_balance_logdirs on the GPU.
    Returns (result, restatement)."""
    c = dict(dir_start=np.asarray(c["dir_start"], dtype=np.int64), dir=np.asarray(c["dir"], dtype=np.int64), size=np.asarray(c["size"], dtype=np.int64), base=c.get("base"))
    ref = lx.descend(c["dir_start"], c["dir"], c["size"], c["base"], min_gain, max_rounds) if ref is None else ref
    rc, res = _abi(lib, "kao_balance_logdirs_exchange", c, min_gain, max_rounds)
    assert rc == 0, lib.kao_last_error().decode()
    print(f"B={len(c['dir_start']) - 1} R={len(c['dir'])} gpu={[res[k] for k in NUMBERS if k != 'per_broker']} stats={res['stats']} ref={ref['stats']}")
    assert res["dir"].tobytes() == ref["dir"].tobytes()
    assert all(res[k] == ref[k] for k in NUMBERS), [(k, res[k], ref[k]) for k in NUMBERS if res[k] != ref[k]][:3]
    assert res["stats"][:4] == ref["stats"][:4] and res["stats"][5:] == ref["stats"][5:] and res["stats"][4] in (2, 4)
    rc, dry = _abi(lib, "kao_balance_logdirs_exchange", c, min_gain, max_rounds, dry_run=True)
    assert rc == 0 and (dry["dir"] == c["dir"]).all() and all(dry[k] == res[k] for k in NUMBERS) and dry["stats"] == res["stats"]
    rc, plain = _abi(lib, "kao_balance_logdirs", c, min_gain, 0)   # both calls on the GPU: the peak of every broker is no higher with exchanges
    assert rc == 0
    if res["stats"][5] == 0:
        assert all(p[1] <= q[1] and p[0] == q[0] and p[2] == q[2] for p, q in zip(res["per_broker"], plain["per_broker"]))
        assert lr.stable(c["dir_start"], res["dir"], c["size"], c["base"], min_gain)
        if len(c["dir"]) <= 3000:
            assert lx.exchange_stable(c["dir_start"], res["dir"], c["size"], c["base"], min_gain)
    return res, ref, plain


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(lib):
    """The 120 seeds in one pass."""
    return [_checked(lib, lr.small_case(seed)) for seed in range(120)]


def test_small_family_matches_the_restatement(small):
    x_rounds = sum(res["stats"][8] for res, _, _ in small)
    better = sum(p[1] < q[1] for res, _, plain in small for p, q in zip(res["per_broker"], plain["per_broker"]))
    print(f"exchange rounds: {x_rounds}, brokers with a lower peak than kao_balance_logdirs: {better}")
    assert x_rounds == 92 and better >= 54   # tests/test_logdirs_x_ref.py: 54 of the enumerated brokers


# ---- 2. dir counts -------------------------------------------------------------------------------------------------------------------
def _spread(n_dirs, per_dir, seed):
    """One broker of n_dirs dirs, about per_dir replicas a dir, log-normal sizes, skewed toward the low dirs, a few dirs with a base."""
    rng = np.random.default_rng(seed)
    k = n_dirs * per_dir
    d = lr._skewed_dirs(rng, n_dirs, k)
    size = np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), 0.7, k)))).astype(np.int64)
    base = np.where(rng.random(n_dirs) < 0.2, rng.integers(1, 3 << 20, n_dirs), 0).astype(np.int64)
    return dict(dir_start=np.array([0, n_dirs]), dir=d, size=size, base=base)


@pytest.mark.parametrize("n_dirs", [2, 3, 63, 64])
def test_dir_counts(lib, n_dirs):
    c = _spread(n_dirs, 6 if n_dirs > 3 else 20, n_dirs)
    ref = lx.descend(**c)
    assert ref["stats"][8] > 0 and ref["stats"][9] > 0   # exchange rounds occur
    _checked(lib, c, ref=ref)


# ---- 3. bucket sizes -----------------------------------------------------------------------------------------------------------------
def _bucket(k):
    return lr.lognormal_case(1, 4, k, 0.7, k)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 256, 257, 1024, 1025, 4095, 4096, 4097])
def test_bucket_sizes(lib, k):
    """One broker with k replicas on 4 dirs: both workgroup sizes (up to 1,024 replicas and beyond), PI and the masks in LDS (up to
    4,096 replicas on 4 dirs) and in global memory (4,097), and the word edges of a mask."""
    res, ref, _ = _checked(lib, _bucket(k))
    assert k < 63 or (res["stats"][8] > 0 and res["stats"][9] > 0)


@pytest.mark.parametrize("k", [1025, 4096])
def test_forced_paths_give_the_same_bytes(lib, k):
    """1,025 replicas and the most that the LDS path holds on 4 dirs, each in LDS and in global memory."""
    c = _bucket(k)
    ref = lx.descend(**c)
    try:
        for path in (1, 2):
            assert lib.kao_logdirs_test_exchange(path) in (0, 1, 2)
            _checked(lib, c, ref=ref)
        rc, _ = _abi(lib, "kao_balance_logdirs_exchange", _bucket(4097))   # still forced to global memory: fine
        assert rc == 0
        lib.kao_logdirs_test_exchange(1)
        rc, _ = _abi(lib, "kao_balance_logdirs_exchange", _bucket(4097))   # forced into LDS: refused, not run
        assert rc == -2 and "LDS" in lib.kao_last_error().decode()
    finally:
        lib.kao_logdirs_test_exchange(0)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------
def test_equal_sizes_are_the_plain_call(lib):
    """Every positive size equal: no exchange exists, the call is kao_balance_logdirs in every shared place, on the GPU."""
    rng = np.random.default_rng(3)
    size = np.where(rng.random(600) < 0.1, 0, 4096).astype(np.int64)
    c = dict(dir_start=np.array([0, 5, 8]), dir=np.concatenate([lr._skewed_dirs(rng, 5, 400), 5 + lr._skewed_dirs(rng, 3, 200)]), size=size, base=None)
    res, ref, plain = _checked(lib, c)
    assert res["stats"][8:] == [0, 0, 0, 0] and res["n_moved"] > 0
    assert res["dir"].tobytes() == plain["dir"].tobytes() and all(res[k] == plain[k] for k in NUMBERS if k != "per_broker")
    assert [p[:6] for p in res["per_broker"]] == plain["per_broker"] and res["stats"][:4] == plain["stats"][:4] and res["stats"][5:8] == plain["stats"][5:]


def test_bases_zero_sizes_and_tied_loads(lib):
    c = lr.lognormal_case(6, 5, 60, 0.7, 11, zeros=0.3, based=0.6)   # bases present, a third of the replicas empty: never a partner
    res, ref, _ = _checked(lib, c)
    assert res["stats"][8] > 0
    moved = res["dir"] != np.asarray(c["dir"])
    assert not (moved & (c["size"] == 0)).any()
    res, _, _ = _checked(lib, dict(dir_start=[0, 2], dir=[0, 0, 1, 1], size=[6, 4, 7, 3], base=None))   # L = (10, 10): D = 0 is skipped
    assert res["stats"][1] == 0 and res["stats"][10] == 0
    res, _, _ = _checked(lib, dict(dir_start=[0, 2], dir=[0, 0, 1, 1], size=[6, 0, 0, 4], base=None))   # the 0 on dir 1 is no partner for the 6
    assert res["stats"][1] == 0
    res, _, _ = _checked(lib, dict(dir_start=[0, 2], dir=[0, 0, 0, 1, 1, 1], size=[10, 7, 4, 8, 5, 4], base=[5, 5]))   # tests/test_logdirs_x_ref.py, on bases
    assert res["per_broker"] == [[26, 24, 24, 2, 18, 1, 1, 1]] and res["stats"][8:] == [1, 1, 2, 1]


def test_min_gain_and_max_rounds(lib):
    c = lr.lognormal_case(1, 4, 40, 0.7, 7)
    full, _, plain = _checked(lib, c)
    m = plain["stats"][1]
    cut, _, _ = _checked(lib, c, max_rounds=m)          # cut at the last move round: kao_balance_logdirs
    assert cut["dir"].tobytes() == plain["dir"].tobytes() and cut["stats"][5] == 1 and cut["stats"][8] == 0
    one, _, _ = _checked(lib, c, max_rounds=m + 1)      # one round more: the first exchange round only
    assert one["stats"][8] == 1 and int((one["dir"] != plain["dir"]).sum()) == 2 * one["stats"][9]
    for mg in (1, 4096, 2 ** 20, 2 ** 62, 2 ** 64 - 1):
        res, _, _ = _checked(lib, c, min_gain=mg)
        assert mg < 2 ** 62 or res["stats"][1] == 0
    hand = dict(dir_start=[0, 2], dir=[0, 0, 0, 1, 1, 1], size=[10, 7, 4, 8, 5, 4], base=None)
    assert [_checked(lib, hand, min_gain=mg)[0]["stats"][9] for mg in (0, 1, 2, 3)] == [1, 1, 0, 0]   # at, below and above the decisive D - delta = 2


# ---- 5. many brokers -----------------------------------------------------------------------------------------------------------------
def test_many_brokers_are_independent(lib):
    """300 brokers of mixed dir counts in one call: every broker's row and dirs are those of the same broker called alone."""
    rng = np.random.default_rng(21)
    nd = rng.choice([0, 1, 2, 3, 4, 6, 12], size=300)
    ds = np.concatenate([[0], np.cumsum(nd)]).astype(np.int64)
    parts = [ds[b] + lr._skewed_dirs(rng, int(n), int(rng.integers(0, 12 * n))) for b, n in enumerate(nd) if n]
    d = np.concatenate(parts).astype(np.int64)
    rng.shuffle(d)
    size = np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), 0.7, len(d))))).astype(np.int64)
    size[rng.random(len(d)) < 0.05] = 0
    D = int(ds[-1])
    c = dict(dir_start=ds, dir=d, size=size, base=np.where(rng.random(D) < 0.3, rng.integers(1, 4 << 20, D), 0).astype(np.int64))
    res, ref, _ = _checked(lib, c)
    assert res["stats"][8] > 100 and res["stats"][11] > 50
    for b in range(300):
        one, mine = lr.one_broker(c, b)
        if len(mine) == 0:
            continue
        rc, alone = _abi(lib, "kao_balance_logdirs_exchange", one)
        assert rc == 0
        # alone, the keys carry other r: the same order inside the broker (mine is ascending), so the same winners
        assert alone["per_broker"][0] == res["per_broker"][b] and (alone["dir"] + int(ds[b]) == res["dir"][mine]).all()


def test_invalid_arguments_leave_dir_alone(kao):
    """Every refusal of include/kao.h is one on a machine with a device too."""
    import test_logdirs_errors as shared
    import test_logdirs_x_errors as host
    for what, change, code, text in shared.REFUSED:
        rc, msg = host._call(**change)
        assert rc == code and text in msg, what


# ---- 6. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-logdirs")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.logdirs"])


def test_cli_against_python(kao, tmp_path):
    """cli/kao-logdirs and the Python twin with --exchange: the same plan file, the same report, both the library's; and the refused
    combinations."""
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs, balance_logdirs_arrays, parse_input
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(8)
    ids = [10 + 2 * i for i in range(6)]
    ndirs = {b: int(rng.integers(2, 5)) for b in ids}
    doc, held = {"version": 1, "partitions": []}, {b: [[] for _ in range(ndirs[b])] for b in ids}
    for name, P, rf in (("alpha", 40, 3), ("beta", 25, 2)):
        for p in range(P):
            r = rng.permutation(6)[:rf]
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
            w = int(np.exp(rng.normal(np.log(2.0 ** 20), 0.7)))
            for b in r:
                i = 0 if rng.random() < 0.6 else int(rng.integers(0, ndirs[ids[b]]))
                held[ids[b]][i].append({"partition": f"{name}-{p}", "size": w + int(b), "offsetLag": 0, "isFuture": False})
    logdirs = {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": f"/data/d{i}", "error": None, "partitions": e} for i, e in enumerate(held[b])]} for b in ids]}
    cur_path, dirs_path = tmp_path / "current.json", tmp_path / "logdirs.txt"
    cur_path.write_text(json.dumps(doc))
    dirs_path.write_text(json.dumps(logdirs) + "\n")
    base = ["--current", str(cur_path), "--log-dirs", str(dirs_path)]
    for tag, flags, kw in (("x", ["--exchange"], {}), ("gain", ["--exchange", "--min-gain", "4K"], dict(min_gain=4096)), ("dry", ["--exchange", "--dry-run"], dict(dry_run=True))):
        outs = []
        for i, prog in enumerate(PROGS):
            out = tmp_path / f"{tag}{i}.json"
            r = subprocess.run(prog + base + flags + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
            assert r.returncode == 0, r.stderr
            outs.append((out.read_bytes(), r.stderr.decode()))
        assert outs[0] == outs[1]
        lib_plan = balance_logdirs(doc, dirs_path.read_text(), exchange=True, **kw)
        res, report = lib_plan.result, outs[0][1].splitlines()
        assert outs[0][0].decode() == lib_plan.text() and report == lib_plan.report_lines() and json.loads(outs[0][0]) == lib_plan.document()
        li = parse_input(doc, dirs_path.read_text())
        arrays = balance_logdirs_arrays(li.dir_start, li.dir, li.size, li.base, exchange=True, **kw)
        assert arrays.dir.tobytes() == res.dir.tobytes() and arrays.per_broker.tobytes() == res.per_broker.tobytes() and arrays.stats.tolist() == res.stats.tolist()
        assert res.per_broker.shape == (6, 8) and res.stats.shape == (12,) and res.stats[8] > 0
        assert all(f" exchange_rounds={int(res.per_broker[i, 6])} exchanges={int(res.per_broker[i, 7])}" in report[i] for i in range(6))
        assert report[-1].endswith(f" exchange_rounds={res.stats[8]} exchanges={res.stats[9]} exchange_proposals={res.stats[10]} brokers_lowered_by_exchange={res.stats[11]}")
        plain = balance_logdirs(doc, dirs_path.read_text(), **kw)
        assert (res.per_broker[:, 1] <= plain.result.per_broker[:, 1]).all() and "exchange" not in plain.report_lines()[-1]
    (tmp_path / "caps.json").write_text("{}")
    for prog in PROGS:
        for bad in (["--utilisation"], ["--capacities", str(tmp_path / "caps.json")], ["--default-capacity", "1G"], ["--plan", str(cur_path)],
                    ["--evacuate", f"{ids[0]}:/data/d0"], ["--plan", str(cur_path), "--rebalance"]):
            r = subprocess.run(prog + base + ["--exchange", "--out", str(tmp_path / "no.json")] + bad, capture_output=True, cwd=ROOT)
            assert r.returncode == 2 and b"--exchange cannot be combined" in r.stderr and not (tmp_path / "no.json").exists(), bad
