"""CPU tests of leader-only rebalancing (kao_balance_leaders): the two host restatements of
tests/leaders_ref.py -- successive shortest paths one path at a time, and the kernels' phases step by step -- against the HiGHS LP
of the restricted model on the small random family and on the ring family; the entry point is declared, exported and bound, rejects
bad input before touching a device and fails loudly without one; the command-line tool's usage and input errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import leaders_ref as lr
from conftest import ROOT, have_gpu

NONE = 0xFFFF


def test_restatements_match_highs_on_the_small_family():
    infeasible = 0
    for i, (rows, B, lo, hi) in enumerate(lr.small_family()):
        opt = lr.lp_optimum(rows, B, lo, hi)
        ok1, out1, n1 = lr.balance_ref(rows, B, lo, hi)
        ok2, out2, n2, stats = lr.kernel_model(rows, B, lo, hi)
        if opt is None:
            infeasible += 1
            assert not ok1 and not ok2 and n1 == n2 == 0 and stats[7] > 0, i
            assert (out1 == rows).all() and (out2 == rows).all(), i
            continue
        assert ok1 and ok2 and n1 == n2 == opt, (i, opt, n1, n2)
        for out, n in ((out1, n1), (out2, n2)):
            assert lr.check_swap(rows, out) == n, i
            cnt = np.bincount(out[:, 0], minlength=B)
            assert cnt.min() >= lo and cnt.max() <= hi, i
        assert stats[2] == stats[4] + max(0, int(np.clip(np.bincount(rows[:, 0], minlength=B), lo, hi).sum()) - rows.shape[0]), i
    assert 10 <= infeasible <= 100, infeasible


@pytest.mark.parametrize("seed,B,P", lr.RING_CASES)
def test_restatements_match_highs_on_the_ring_family(seed, B, P):
    rows, B, lo, hi = lr.ring_instance(seed, B, P)
    opt = lr.lp_optimum(rows, B, lo, hi)
    assert opt == lr.RING_LP[(seed, B)]
    ok1, out1, n1 = lr.balance_ref(rows, B, lo, hi)
    ok2, out2, n2, stats = lr.kernel_model(rows, B, lo, hi)
    assert ok1 and ok2 and n1 == n2 == opt
    assert lr.check_swap(rows, out1) == n1 and lr.check_swap(rows, out2) == n2
    assert stats[3] >= 2 and stats[7] == 0   # leadership travels over several arcs


def _topic(B, rows, **over):
    from kafka_assignment_optimizer_amd import Topic
    rows = np.asarray(rows, dtype=np.uint16)
    return Topic(name="t", broker_ids=np.arange(B), rack_of=np.arange(B) % 2, n_racks=2, n_partitions=rows.shape[0], rf=rows.shape[1],
                 current=rows, bounds_override=dict(over))


def _call(topic, rows, null=None):
    from kafka_assignment_optimizer_amd import _ffi
    from kafka_assignment_optimizer_amd.solver import _CTopics
    ct = _CTopics([topic])
    a = np.ascontiguousarray(rows, dtype=np.uint16).reshape(-1).copy()
    n, status = C.c_int32(0), C.c_int32(0)
    args = [ct.arr, a.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(n), None, C.byref(status), None]
    if null is not None:
        args[null] = None
    return _ffi.load().kao_balance_leaders(*args)


def test_balance_leaders_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_leaders\(const kao_topic \*t, uint16_t \*assignment /\* \[P\*rf\] in / out \*/, int32_t \*n_changed,\s+"
                     r"int64_t \*objective /\* [^*]* \*/,\s+int32_t \*status, int32_t stats\[8\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header
    res, args = _ffi.SIGNATURES["kao_balance_leaders"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [P(_ffi.KaoTopic), P(C.c_uint16), P(C.c_int32), P(C.c_int64), P(C.c_int32), P(C.c_int32)]
    fn = _ffi.load().kao_balance_leaders
    assert fn.argtypes == args and fn.restype is C.c_int


def test_balance_leaders_rejects_bad_input():
    """KAO_ERR_INVALID (-1) for every malformed call, checked on the host before any device is used."""
    rows = np.array([[0, 1], [2, 3], [1, 2]])
    t = _topic(4, rows)
    for null in (0, 1, 2, 4):                                         # topic, assignment, n_changed, status
        assert _call(t, rows, null=null) == -1
    assert _call(t, np.array([[0, 1], [2, 4], [1, 2]])) == -1         # broker index >= n_brokers
    assert _call(t, np.array([[0, 1], [2, NONE], [1, 2]])) == -1      # incomplete row
    assert _call(t, np.array([[0, 1], [3, 3], [1, 2]])) == -1         # broker twice in a row
    assert _call(_topic(4, rows, lead_lo=2, lead_hi=1), rows) == -1   # empty band
    big = np.zeros((1, 2), dtype=np.uint16)
    from kafka_assignment_optimizer_amd import Topic
    huge = Topic(name="t", broker_ids=np.arange(4), rack_of=np.arange(4) % 2, n_racks=2, n_partitions=2000001, rf=2,
                 current=np.tile(np.array([0, 1], dtype=np.uint16), (2000001, 1)), weights=((1, 1), (1, 1)))
    assert _call(huge, big) == -2                                     # more than 4,000,000 replica slots: KAO_ERR_UNSUPPORTED, before a row is read


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_balance_leaders_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.leaders import balance_leaders
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    assert _call(_topic(3, rows), rows) == -3   # KAO_ERR_NO_DEVICE
    with pytest.raises(kao.KaoError) as e:
        balance_leaders(_topic(3, rows))
    assert e.value.code == -3


def test_python_front_end_checks_its_arguments():
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders, plan_text
    t = Topic(name="t", broker_ids=np.arange(3), rack_of=np.zeros(3), n_racks=1, n_partitions=2, rf=3, current=np.array([[0, 1], [1, 2]]))
    with pytest.raises(ValueError, match="rf_cur"):
        balance_leaders(t)
    with pytest.raises(ValueError, match="P\\*rf"):
        balance_leaders(t, np.zeros((2, 2)))
    assert plan_text([]) == '{"version":1,"partitions":[\n]}\n'
    assert plan_text([("a", 1, [2, 0]), ("a", 3, [1, 2])]) == \
        '{"version":1,"partitions":[\n    {"topic":"a","partition":1,"replicas":[2,0]},\n    {"topic":"a","partition":3,"replicas":[1,2]}\n]}\n'


def test_cli_usage_and_input_errors(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "cli", "kao-leaders")
    assert subprocess.run([exe], capture_output=True).returncode == 2
    assert subprocess.run([exe, "--bogus"], capture_output=True).returncode == 2
    base = ["--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a"]
    assert subprocess.run([exe, "--current", "c.json", "--slack", "-1"] + base, capture_output=True).returncode == 2
    r = subprocess.run([exe, "--current", "/nonexistent.json"] + base, capture_output=True)
    assert r.returncode == 1 and b"cannot open" in r.stderr
    cur = tmp_path / "cur.json"
    cur.write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"replicas":[0,1]},{"topic":"a","partition":7,"replicas":[2,5]}]}')
    r = subprocess.run([exe, "--current", str(cur)] + base, capture_output=True)   # broker 5 is outside the list
    assert r.returncode == 1 and b"a-7" in r.stderr and b"kao-cli" in r.stderr
