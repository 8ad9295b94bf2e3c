"""CPU tests of the traffic-weighted failover order (kao_failover_order_weighted): the restatement of the rounds
in tests/wfailover_ref.py ends move-stable and is bracketed by the certificate and the exact optimum on the tiny family (every choice
tried) and on the small family (HiGHS); with unit weights it brackets the exact answer of section 4i; the entry point is declared,
exported and bound, rejects bad input before touching a device and fails loudly without one; the Python front end's argument checks
and both command-line tools' usage errors."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import failover_ref as fr
import wfailover_ref as wf
from conftest import ROOT, have_gpu

NONE = 0xFFFF


@pytest.fixture(autouse=True, scope="module")
def bound():
    """The reference restates an entry point: without it there is nothing to hold it against."""
    from kafka_assignment_optimizer_amd import _ffi
    assert "kao_failover_order_weighted" in _ffi.SIGNATURES
    return _ffi.load().kao_failover_order_weighted


def _bracket(family, weights_of, exact_up_to):
    """Every scenario of every instance in both scopes: rows one swap away from the input, no move left, the bound recomputed from
    the returned rows, lower_bound <= optimum <= peak_after <= peak_before.  Returns the counts over the scenarios with work."""
    c = dict(scenarios=0, improved=0, proven=0, at_optimum=0, most_rounds=0)
    for i, (rows, B, rack_of, R) in enumerate(family):
        w = weights_of(i, len(rows))
        for scope in (0, 1):
            res = wf.descend(rows, w, B, rack_of, scope, R)
            assert fr.check_rows(rows, res["rows"], B, rack_of, scope) == res["n_reordered"], (i, scope)
            assert wf.stable(res["rows"], w, B, rack_of, scope), (i, scope)
            assert wf.lower_bound(res["rows"], w, B, rack_of, scope, R) == [s[4] for s in res["scen"]], (i, scope)
            opt = wf.optimum(rows, w, B, rack_of, scope, R, enumerate_up_to=exact_up_to)
            for g, (aff, off, before, after, lb, re_) in enumerate(res["scen"]):
                assert lb <= opt[g] <= after <= before, (i, scope, g, res["scen"][g], opt[g])
                if aff == 0:
                    assert lb == after == before and re_ == 0
                    continue
                c["scenarios"] += 1
                c["improved"] += after < before
                c["proven"] += after == lb
                c["at_optimum"] += after == opt[g]
            assert res["proven"] == all(s[3] == s[4] for s in res["scen"])
            assert res["stats"][5] == 0 and res["stats"][2] >= res["stats"][1] and res["stats"][3] >= res["stats"][2]
            c["most_rounds"] = max(c["most_rounds"], res["stats"][7])
    return c


def test_restatement_against_every_choice_on_the_tiny_family():
    """failover_ref.tiny_family() with wfailover_ref.family_weights (default_rng(500 + i); integers 0..49 on even i, a rounded
    log-normal on odd i), both scopes, the optimum by trying every choice.  This seeding gives 459 scenarios with work: 100 improve,
    439 are proven (peak_after == lower_bound), 454 end at the optimum, and no scenario runs more than 4 rounds."""
    c = _bracket(fr.tiny_family(), wf.family_weights, exact_up_to=7)
    print(c)
    assert c["improved"] >= 1 and c["proven"] >= 1 and c["proven"] < c["scenarios"]
    assert c["at_optimum"] >= c["proven"]


def test_restatement_against_highs_on_the_small_family():
    """failover_ref.small_family() with log-normal weights (family_weights(2 i + 1)), the optimum by HiGHS above 7 affected
    partitions.  This seeding gives 956 scenarios with work: 302 improve, 922 are proven, the most rounds of one scenario is 9."""
    c = _bracket(fr.small_family(), lambda i, P: wf.family_weights(2 * i + 1, P), exact_up_to=7)
    print(c)
    assert c["scenarios"] == 956 and c["improved"] >= 1 and 1 <= c["proven"] < c["scenarios"]


def test_unit_weights_bracket_the_exact_failover_order():
    """With weight 1 everywhere L_g counts leaders: peak_before is failover_ref.simulate's peak and the exact optimum of section 4i
    lies between the bound and the descent's peak."""
    improved = 0
    for (rows, B, rack_of, R), optima in zip(fr.small_family()[:40], fr.small_family_optima()[:40]):
        for scope in (0, 1):
            res = wf.descend(rows, np.ones(len(rows), dtype=np.int64), B, rack_of, scope, R)
            sim = fr.simulate(rows, B, rack_of, scope, R)
            for g, s in enumerate(res["scen"]):
                assert s[:3] == sim[g].tolist(), (scope, g)
                assert s[4] <= optima[scope][g, 3] <= s[3], (scope, g, s, optima[scope][g])
                improved += s[3] < s[2]
    assert improved > 0


def test_contention_shapes_and_limits():
    for B in (3, 4, 5):
        rows, w, B, rack_of, R = wf.contention_case(B, 64)
        res = wf.descend(rows, w, B, rack_of, 0, R)
        assert res["scen"][0][:3] == [64, 0, 64 * 5] and res["stats"][0] == 1 and wf.stable(res["rows"], w, B, rack_of, 0)
        assert res["scen"][0][3] == -(-64 // (B - 1)) * 5   # equal weights: stable means within one weight of even
        one = wf.descend(rows, w, B, rack_of, 0, R, max_rounds=1)
        assert one["stats"][1] == 1 and one["stats"][2] == 1 and one["stats"][5] == 1   # one source: one winner per round
        none = wf.descend(rows, w, B, rack_of, 0, R, min_gain=64 * 5)
        assert none["stats"][:4] == [1, 0, 0, 0] and none["n_reordered"] == 0 and (none["rows"] == rows).all()


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def _call(rows, B=4, R=2, rack_of=(0, 1, 0, 1), weight=(5, 6, 7), scope=0, min_gain=0, max_rounds=0, null=None, P=None, W=None):
    from kafka_assignment_optimizer_amd import _ffi
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    rk = np.ascontiguousarray(rack_of, dtype=np.uint8)
    wt = np.ascontiguousarray(weight, dtype=np.uint64)
    scen = np.zeros((max(B, R, 1), 6), dtype=np.uint64)
    n, status = C.c_int32(0), C.c_int32(0)
    args = [B, R, rk.ctypes.data_as(C.POINTER(C.c_uint8)), r.shape[0] if P is None else P, r.shape[1] if W is None else W,
            r.ctypes.data_as(C.POINTER(C.c_uint16)), wt.ctypes.data_as(C.POINTER(C.c_uint64)), scope, min_gain, max_rounds, 0,
            scen.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n), C.byref(status), None]
    if null is not None:
        args[null] = None
    rc = _ffi.load().kao_failover_order_weighted(*args)
    assert (r == keep).all()   # a rejected call leaves the rows alone
    return rc


def test_entry_point_is_declared_exported_and_bound(bound):
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_failover_order_weighted\(int32_t n_brokers, int32_t n_racks, const uint8_t \*rack_of, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/, const uint64_t \*weight /\* \[n_partitions\] \*/,\s+"
                     r"int32_t scope, uint64_t min_gain, int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run,\s+"
                     r"uint64_t \*scen /\* \[n_scen\*6\] \*/, int32_t \*n_reordered, int32_t \*status,\s+"
                     r"int64_t stats\[8\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header
    res, args = _ffi.SIGNATURES["kao_failover_order_weighted"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [C.c_int32, C.c_int32, P(C.c_uint8), C.c_int32, C.c_int32, P(C.c_uint16), P(C.c_uint64), C.c_int32, C.c_uint64, C.c_int32,
                    C.c_int32, P(C.c_uint64), P(C.c_int32), P(C.c_int32), P(C.c_int64)]
    assert bound.argtypes == args and bound.restype is C.c_int


ROWS = [[0, 1, 2], [2, 3, NONE], [1, NONE, NONE]]
INVALID = [
    ("null rack_of", dict(null=2)), ("null rows", dict(null=5)), ("null weight", dict(null=6)), ("null scen", dict(null=11)),
    ("null n_reordered", dict(null=12)), ("null status", dict(null=13)),
    ("scope -1", dict(scope=-1)), ("scope 2", dict(scope=2)), ("width 0", dict(W=0)), ("width above KAO_MAX_RF", dict(W=9)),
    ("no broker", dict(B=0, rack_of=[0])), ("too many brokers", dict(B=65535, rack_of=np.zeros(65535))),
    ("no rack", dict(R=0)), ("too many racks", dict(R=256)), ("rack_of >= n_racks", dict(R=1)), ("negative partitions", dict(P=-1)),
    ("slot 0 empty", dict(rows=[[NONE, 1, 2]], weight=[1])), ("a broker after an empty slot", dict(rows=[[0, NONE, 2]], weight=[1])),
    ("index >= n_brokers", dict(rows=[[0, 1, 4]], weight=[1])), ("broker twice", dict(rows=[[0, 1, 0]], weight=[1])),
    ("weights sum to 2^62", dict(weight=[2 ** 61, 2 ** 61, 0])), ("weights sum past 2^64", dict(weight=[2 ** 63, 2 ** 63, 5])),
    ("one weight of 2^62", dict(weight=[0, 2 ** 62, 0])),
]


@pytest.mark.parametrize("what,change", INVALID, ids=[w for w, _ in INVALID])
def test_entry_point_rejects_bad_input(what, change):
    """KAO_ERR_INVALID (-1), checked on the host before any device is used; the rows stay as they are."""
    kw = dict(rows=ROWS)
    kw.update(change)
    assert _call(**kw) == -1


def test_entry_point_reports_unsupported_sizes():
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    limit = int(re.search(r"#define KAO_FAILOVER_MAX_BROKERS (\d+)", header).group(1))
    assert limit == 8000
    assert _call(ROWS, B=limit + 1, rack_of=np.zeros(limit + 1)) == -2     # 8,001 brokers
    assert _call(ROWS, P=4000001, W=1) == -2                               # 4,000,001 slots, before a row or a weight is read
    assert _call(ROWS, P=2000001, W=2) == -2


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.failover import failover_order_weighted_arrays
    assert _call(ROWS) == -3   # KAO_ERR_NO_DEVICE
    assert _call(ROWS, weight=[2 ** 61 - 1, 2 ** 61, 0]) == -3   # just below 2^62 passes the host checks
    assert _call(ROWS, B=8000, rack_of=np.zeros(8000)) == -3
    with pytest.raises(kao.KaoError) as e:
        failover_order_weighted_arrays(ROWS, 4, [0, 1, 0, 1], 2, "rack", [5, 6, 7])
    assert e.value.code == -3


# ---- the Python front end and the command-line tools -------------------------------------------------------------------------------
def test_python_front_end_checks_its_arguments():
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd import failover as fo
    rows = np.array([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="scope"):
        fo.failover_order_weighted_arrays(rows, 3, np.zeros(3), 1, "zone", [1, 1])
    with pytest.raises(ValueError, match="width"):
        fo.failover_order_weighted_arrays(rows.reshape(-1), 3, np.zeros(3), 1, 0, [1, 1, 1, 1])
    with pytest.raises(ValueError, match="rack_of"):
        fo.failover_order_weighted_arrays(rows, 3, np.zeros(2), 1, 0, [1, 1])
    with pytest.raises(ValueError, match="one value per row"):
        fo.failover_order_weighted_arrays(rows, 3, np.zeros(3), 1, 0, [1])
    with pytest.raises(ValueError, match=">= 0"):
        fo.failover_order_weighted_arrays(rows, 3, np.zeros(3), 1, 0, [1, -1])
    with pytest.raises(ValueError, match="integers"):
        fo.failover_order_weighted_arrays(rows, 3, np.zeros(3), 1, 0, [1.5, 2.0])
    with pytest.raises(ValueError, match="min_gain"):
        fo.failover_order_weighted_arrays(rows, 3, np.zeros(3), 1, 0, [1, 2], min_gain=-1)
    with pytest.raises(ValueError, match="broker_list"):
        fo.failover_order_weighted({"partitions": []}, "broker", {})
    with pytest.raises(ValueError, match="no topic"):
        fo.failover_order_weighted([], "broker", {})
    a = Topic(name="a", broker_ids=np.arange(3), rack_of=np.zeros(3), n_racks=1, n_partitions=2, rf=2, current=rows)
    b = Topic(name="b", broker_ids=np.arange(4), rack_of=np.zeros(4), n_racks=1, n_partitions=2, rf=2, current=rows)
    with pytest.raises(ValueError, match="one broker index"):
        fo.failover_order_weighted([a, b], "broker", {}, default_weight=1)
    with pytest.raises(ValueError, match="distinct"):
        fo.failover_order_weighted([a, a], "broker", {}, default_weight=1)
    with pytest.raises(ValueError, match="no weight for partitions a-1"):
        fo.failover_order_weighted([a], "broker", {("a", 0): 4})
    with pytest.raises(ValueError, match="one array"):
        fo.failover_order_weighted([a], "rack", [[1, 2, 3]])
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 1, "replicas": [7, 5, 6]}]}
    with pytest.raises(ValueError, match="one array"):
        fo.failover_order_weighted(doc, "rack", [[1]], broker_list=[5, 6, 7], racks={5: "x", 6: "y", 7: "x"})
    with pytest.raises(ValueError, match="no weight for partitions t-1"):
        fo.failover_order_weighted(doc, "rack", {("t", 0): 3}, broker_list=[5, 6, 7], racks={5: "x", 6: "y", 7: "x"})


PROGS = ([os.path.join(ROOT, "cli", "kao-failover")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.failover"])


def test_cli_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    base = ["--current", str(tmp_path / "c.json"), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--scope", "broker"]
    t, s = ["--traffic", str(tmp_path / "t.json")], ["--sizes", str(tmp_path / "s.txt")]
    usage = [t + s, ["--default-weight", "3"], ["--min-gain", "3"], ["--max-rounds", "3"], ["--dry-run", "--min-gain", "3"],
             t + ["--default-weight", "-1"], t + ["--default-weight", "x"], t + ["--default-weight", str(2 ** 53 + 1)], t + ["--min-gain", "-2"],
             t + ["--min-gain", str(2 ** 64)], t + ["--max-rounds", "-1"], t + ["--max-rounds", "1.5"], ["--traffic"], t + ["--min-gain"]]
    for prog in PROGS:
        for extra in usage:
            r = subprocess.run(prog + base + extra, capture_output=True, cwd=ROOT)
            assert r.returncode == 2, (prog, extra, r.stderr)
        r = subprocess.run(prog + base + t, capture_output=True, cwd=ROOT)   # the document does not exist
        assert r.returncode == 1, (prog, r.stderr)
    (tmp_path / "c.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"replicas":[0,1]},{"topic":"b","partition":7,"replicas":[2,1]}]}')
    (tmp_path / "t.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"weight":5}]}')
    (tmp_path / "dup.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"weight":5},{"topic":"a","partition":0,"weight":5}]}')
    (tmp_path / "neg.json").write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"weight":-5}]}')
    for prog in PROGS:
        r = subprocess.run(prog + base + t, capture_output=True, cwd=ROOT)   # b-7 has no weight and there is no default
        assert r.returncode == 1 and b"no weight for partitions b-7" in r.stderr, (prog, r.stderr)
        r = subprocess.run(prog + base + ["--traffic", str(tmp_path / "dup.json")], capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"a-0 listed twice" in r.stderr, (prog, r.stderr)
        r = subprocess.run(prog + base + ["--traffic", str(tmp_path / "neg.json")], capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"weight must be an integer 0..2^53" in r.stderr, (prog, r.stderr)
