"""CPU tests of the traffic-weighted leader balance (kao_balance_leaders_weighted): the restatement of the
rounds in tests/wleaders_ref.py terminates, ends move-stable and is bracketed by the certificate and the exact optimum (HiGHS) on
the small family; the entry point is declared, exported and bound, rejects bad input before touching a device and fails loudly
without one; the traffic document, the Python front end's argument checks and the command-line tools' usage errors."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import wleaders_ref as wr
from conftest import ROOT, have_gpu, load_golden

NONE = 0xFFFF
SEEDS = range(120)


@pytest.fixture(autouse=True, scope="module")
def bound():
    """The reference restates an entry point: without it there is nothing to hold it against."""
    from kafka_assignment_optimizer_amd import _ffi
    assert "kao_balance_leaders_weighted" in _ffi.SIGNATURES
    return _ffi.load().kao_balance_leaders_weighted


def test_code_is_monotone_and_matches_its_scalar_form():
    xs = [0, 1, 2, 3, 5, 511, 512, 513, 1023, 1024, 1025, 2 ** 20, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7, 2 ** 48, 2 ** 48 + 2 ** 39, 2 ** 62 - 1]
    got = wr.code(np.array(xs, dtype=np.uint64)).tolist()
    assert got == [wr.code_scalar(x) for x in xs]
    assert got == sorted(got) and got[0] == 0 and got[1] == 1 << 9 and max(got) < 1 << 16


def test_restatement_is_stable_and_bracketed_on_the_small_family():
    """lower_bound <= optimum <= peak_after <= peak_before on 120 seeds; the descent ends with no move left.  How often the descent
    reaches the optimum and how often the certificate does is printed: a measurement, not a requirement."""
    at_opt = lb_at_opt = proven = moved = padded = equal = 0
    for seed in SEEDS:
        rows, weight, B = wr.small_case(seed)
        res = wr.descend(rows, weight, B)
        assert wr.stable(rows, res["rows"], weight, B), seed
        assert res["moves"] >= res["rounds"] and res["proposals"] >= res["moves"] and not res["more"], seed
        lb, k = wr.lower_bound(res["rows"], weight, B)
        opt = wr.optimum(rows, weight, B)
        assert lb <= opt <= res["peak_after"] <= res["peak_before"], (seed, lb, opt, res["peak_after"], res["peak_before"])
        assert res["peak_after"] == int(wr.loads(res["rows"], weight, B).max()), seed
        assert res["n_changed"] == int((res["rows"] != rows).any(axis=1).sum()), seed
        at_opt += res["peak_after"] == opt
        lb_at_opt += lb == opt
        proven += res["peak_after"] == lb
        moved += res["n_changed"] > 0
        padded += bool((rows == NONE).any())
        equal += len(set(weight.tolist())) == 1
    print(f"seeds={len(SEEDS)} peak==optimum: {at_opt}  lower_bound==optimum: {lb_at_opt}  proven: {proven}  moved: {moved}")
    assert moved >= 60 and padded >= 100 and equal >= 12   # conditions on the inputs


def test_restatement_on_the_contention_shapes_and_limits():
    for B in (2, 3, 4):
        rows, weight = wr.collide_case(B, 64)
        res = wr.descend(rows, weight, B)
        assert res["peak_before"] == 64 * 5 and wr.stable(rows, res["rows"], weight, B)
        assert res["peak_after"] - int(wr.loads(res["rows"], weight, B).min()) <= 5, B   # equal weights: stable means within one weight
        one = wr.descend(rows, weight, B, max_rounds=1)
        assert one["rounds"] == 1 and one["moves"] == 1 and one["more"]   # one source: one winner per round
        none = wr.descend(rows, weight, B, min_gain=64 * 5)
        assert none["rounds"] == 0 and none["n_changed"] == 0 and (none["rows"] == rows).all()


def test_batch_boundary_case_takes_exactly_one_batch_of_rounds():
    """tests/test_gpu_wleaders.py relies on it: 32 rounds, the batch of the multi-launch path, so its last round with a proposal is
    the last of a batch."""
    res = wr.descend(*wr.lognormal_case(6, 200, 3, 0.7, 26), 6)
    assert res["rounds"] == 32 and not res["more"]


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def _call(rows, B, weight, min_gain=0, max_rounds=0, null=None, P=None, W=None):
    from kafka_assignment_optimizer_amd import _ffi
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    wt = np.ascontiguousarray(weight, dtype=np.uint64)
    n, status = C.c_int32(0), C.c_int32(0)
    u = [C.c_uint64(0) for _ in range(3)]
    args = [B, r.shape[0] if P is None else P, r.shape[1] if W is None else W, r.ctypes.data_as(C.POINTER(C.c_uint16)),
            wt.ctypes.data_as(C.POINTER(C.c_uint64)), min_gain, max_rounds, 0, C.byref(n), C.byref(u[0]), C.byref(u[1]), C.byref(u[2]),
            C.byref(status), None]
    if null is not None:
        args[null] = None
    rc = _ffi.load().kao_balance_leaders_weighted(*args)
    assert (r == keep).all()   # a rejected call leaves the rows alone
    return rc


def test_entry_point_is_declared_exported_and_bound(bound):
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_leaders_weighted\(int32_t n_brokers, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/, const uint64_t \*weight /\* \[n_partitions\] \*/,\s+"
                     r"uint64_t min_gain, int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run,\s+"
                     r"int32_t \*n_changed, uint64_t \*peak_before, uint64_t \*peak_after, uint64_t \*lower_bound,\s+"
                     r"int32_t \*status, int64_t stats\[8\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header
    res, args = _ffi.SIGNATURES["kao_balance_leaders_weighted"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [C.c_int32, C.c_int32, C.c_int32, P(C.c_uint16), P(C.c_uint64), C.c_uint64, C.c_int32, C.c_int32, P(C.c_int32),
                    P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), P(C.c_int32), P(C.c_int64)]
    assert bound.argtypes == args and bound.restype is C.c_int


INVALID = [
    ("null rows", dict(null=3)), ("null weight", dict(null=4)), ("null n_changed", dict(null=8)), ("null peak_before", dict(null=9)),
    ("null peak_after", dict(null=10)), ("null lower_bound", dict(null=11)), ("null status", dict(null=12)),
    ("width 0", dict(W=0)), ("width above KAO_MAX_RF", dict(W=9)), ("no broker", dict(B=0)), ("too many brokers", dict(B=65535)),
    ("negative partitions", dict(P=-1)),
    ("slot 0 empty", dict(rows=[[0, 1], [NONE, 3], [1, 2]])), ("a broker after an empty slot", dict(rows=[[0, NONE, 1], [2, 3, NONE], [1, 2, 0]])),
    ("index >= n_brokers", dict(rows=[[0, 1], [2, 4], [1, 2]])), ("broker twice", dict(rows=[[0, 1], [3, 3], [1, 2]])),
    ("weights sum to 2^62", dict(weight=[2 ** 61, 2 ** 61, 0])), ("weights sum past 2^64", dict(weight=[2 ** 63, 2 ** 63, 5])),
    ("one weight of 2^62", dict(weight=[0, 2 ** 62, 0])),
]


@pytest.mark.parametrize("what,change", INVALID, ids=[w for w, _ in INVALID])
def test_entry_point_rejects_bad_input(what, change):
    """KAO_ERR_INVALID (-1), checked on the host before any device is used; the rows stay as they are."""
    kw = dict(rows=[[0, 1], [2, 3], [1, 2]], B=4, weight=[5, 6, 7])
    kw.update(change)
    assert _call(**kw) == -1


def test_entry_point_reports_unsupported_sizes():
    rows = np.zeros((1, 2), dtype=np.uint16)
    assert _call(rows, 4, [1], P=2000001) == -2   # more than 4,000,000 slots: KAO_ERR_UNSUPPORTED, before a row is read


def test_path_hook_rejects_unknown_paths():
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    assert lib.kao_wleaders_test_path(3) == -1 and lib.kao_wleaders_test_path(-1) == -1
    assert lib.kao_wleaders_test_path(2) == 0 and lib.kao_wleaders_test_path(0) == 2


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_weighted_arrays
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    assert _call(rows, 3, [4, 5, 6]) == -3   # KAO_ERR_NO_DEVICE
    assert _call(rows, 3, [2 ** 61 - 1, 2 ** 61, 0]) == -3   # just below 2^62 passes the host checks
    with pytest.raises(kao.KaoError) as e:
        balance_leaders_weighted_arrays(rows, 3, [4, 5, 6])
    assert e.value.code == -3


# ---- the Python front end and the command-line tools -------------------------------------------------------------------------------
def test_parse_traffic_and_weights_for():
    from kafka_assignment_optimizer_amd.leaders import parse_traffic, weights_for
    table = parse_traffic(load_golden("readme_traffic.json"))
    assert table == {("x.y.z.t", p): w for p, w in enumerate([120, 45, 300, 80, 80, 10, 0, 950, 60, 215])}
    keys = [("x.y.z.t", 7), ("x.y.z.t", 0), ("other", 3)]
    assert weights_for(keys, table, 11).tolist() == [950, 120, 11] and weights_for(keys, table, 11).dtype == np.uint64
    with pytest.raises(ValueError, match="other-3"):
        weights_for(keys, table)
    entry = {"topic": "t", "partition": 1, "weight": 5}
    with pytest.raises(ValueError, match="twice"):
        parse_traffic({"version": 1, "partitions": [entry, dict(entry, weight=6)]})
    for bad in (-1, 1.5, "7", None, True, 2 ** 53 + 1):
        with pytest.raises(ValueError, match="weight must be"):
            parse_traffic({"version": 1, "partitions": [dict(entry, weight=bad)]})
    with pytest.raises(ValueError, match="partitions"):
        parse_traffic({"version": 1})
    assert parse_traffic({"partitions": [dict(entry, weight=2 ** 53)]}) == {("t", 1): 2 ** 53}


def test_python_front_end_checks_its_arguments():
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_weighted, balance_leaders_weighted_arrays
    with pytest.raises(ValueError, match="rows"):
        balance_leaders_weighted_arrays(np.zeros(4), 3, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="one value per row"):
        balance_leaders_weighted_arrays(np.zeros((2, 2)), 3, [1])
    with pytest.raises(ValueError, match=">= 0"):
        balance_leaders_weighted_arrays(np.array([[0, 1], [1, 2]]), 3, [1, -1])
    with pytest.raises(ValueError, match="integers"):
        balance_leaders_weighted_arrays(np.array([[0, 1], [1, 2]]), 3, [1.5, 2.0])
    with pytest.raises(ValueError, match="min_gain"):
        balance_leaders_weighted_arrays(np.array([[0, 1], [1, 2]]), 3, [1, 2], min_gain=-1)
    with pytest.raises(ValueError, match="no topic"):
        balance_leaders_weighted([], {})
    a = Topic(name="a", broker_ids=np.arange(3), rack_of=np.zeros(3), n_racks=1, n_partitions=2, rf=2, current=np.array([[0, 1], [1, 2]]))
    b = Topic(name="b", broker_ids=np.arange(4), rack_of=np.zeros(4), n_racks=1, n_partitions=2, rf=2, current=np.array([[0, 1], [1, 2]]))
    with pytest.raises(ValueError, match="share one broker index"):
        balance_leaders_weighted([a, b], {}, default_weight=1)
    with pytest.raises(ValueError, match="distinct"):
        balance_leaders_weighted([a, a], {}, default_weight=1)
    with pytest.raises(ValueError, match="no weight for partitions a-1"):
        balance_leaders_weighted([a], {("a", 0): 4})
    with pytest.raises(ValueError, match="one array"):
        balance_leaders_weighted([a], [[1, 2, 3]])


def test_cli_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    base = ["--current", str(tmp_path / "c.json"), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a"]
    t, s = ["--traffic", str(tmp_path / "t.json")], ["--sizes", str(tmp_path / "s.txt")]
    usage = [t + s, t + ["--slack", "1"], t + ["--slack", "0"], s + ["--auto-slack"], t + ["--cluster"], s + ["--cluster-lo", "1"],
             t + ["--cluster-hi", "4"], ["--default-weight", "3"], ["--min-gain", "3"], ["--max-rounds", "3"], ["--cluster", "--min-gain", "3"],
             t + ["--default-weight", "-1"], t + ["--default-weight", "x"], t + ["--default-weight", str(2 ** 53 + 1)], t + ["--min-gain", "-2"],
             t + ["--min-gain", str(2 ** 64)], t + ["--max-rounds", "-1"], t + ["--max-rounds", "1.5"], ["--traffic"], t + ["--min-gain"]]
    for prog in ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"]):
        for extra in usage:
            r = subprocess.run(prog + base + extra, capture_output=True, cwd=ROOT)
            assert r.returncode == 2, (prog, extra, r.stderr)
        r = subprocess.run(prog + base + t, capture_output=True, cwd=ROOT)   # the document does not exist
        assert r.returncode == 1, (prog, r.stderr)
    (tmp_path / "c.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"replicas":[0,1]},{"topic":"b","partition":7,"replicas":[2,1]}]}')
    (tmp_path / "t.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"weight":5}]}')
    (tmp_path / "dup.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"weight":5},{"topic":"a","partition":0,"weight":5}]}')
    (tmp_path / "neg.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"weight":-5}]}')
    for prog in ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"]):
        r = subprocess.run(prog + base + t, capture_output=True, cwd=ROOT)   # b-7 has no weight and there is no default
        assert r.returncode == 1 and b"no weight for partitions b-7" in r.stderr, (prog, r.stderr)
        r = subprocess.run(prog + base + ["--traffic", str(tmp_path / "dup.json")], capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"a-0 listed twice" in r.stderr, (prog, r.stderr)
        r = subprocess.run(prog + base + ["--traffic", str(tmp_path / "neg.json")], capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"weight must be an integer 0..2^53" in r.stderr, (prog, r.stderr)


def test_sizes_header_keeps_kao_waves_reading_log_dirs(tmp_path):
    """The log-dirs parser moved into cli/kao_sizes.h: kao-waves still rejects what it rejected, with the same words."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    golden = os.path.join(ROOT, "tests", "golden")
    bad = tmp_path / "sizes.json"
    bad.write_text('{"partitions":[{"topic":"x.y.z.t","partition":1,"size":1.5}]}')
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", os.path.join(golden, "readme_current.json"), "--plan",
                        os.path.join(golden, "readme_proposal.json"), "--out-prefix", str(tmp_path / "w"), "--sizes", str(bad),
                        "--max-bytes-per-broker", "1G"], capture_output=True)
    assert r.returncode == 1 and b"sizes: x.y.z.t-1: size must be an integer 0..2^53" in r.stderr, r.stderr
