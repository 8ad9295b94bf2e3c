"""CPU tests of the wave planner's host layer (kao_plan_waves, kafka_assignment_optimizer_amd/waves.py): the entry point is
declared, exported and bound with the right ctypes signature, rejects bad input before touching a device, fails loudly without
one, and the reassignment documents become rows over the union broker index."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu, load_golden

NONE = 0xFFFF


def _call(B, cur, tgt, k, W=None):
    from kafka_assignment_optimizer_amd import _ffi
    cur = np.ascontiguousarray(cur, dtype=np.uint16)
    tgt = np.ascontiguousarray(tgt, dtype=np.uint16)
    P = cur.shape[0]
    wave = np.zeros(max(P, 1), dtype=np.int32)
    nw, lb = C.c_int32(0), C.c_int32(0)
    u16, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
    return _ffi.load().kao_plan_waves(B, P, cur.shape[1] if W is None else W, cur.ctypes.data_as(u16), tgt.ctypes.data_as(u16), k, 1,
                                      wave.ctypes.data_as(i32), C.byref(nw), C.byref(lb))


def test_plan_waves_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_plan_waves\(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t \*current,\s+"
                     r"const uint16_t \*target,\s+int32_t max_per_broker, uint64_t seed, int32_t \*wave /\* \[n_partitions\] \*/, "
                     r"int32_t \*n_waves, int32_t \*lower_bound\);", header)
    res, args = _ffi.SIGNATURES["kao_plan_waves"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [C.c_int32, C.c_int32, C.c_int32, P(C.c_uint16), P(C.c_uint16), C.c_int32, C.c_uint64, P(C.c_int32), P(C.c_int32),
                    P(C.c_int32)]
    fn = _ffi.load().kao_plan_waves
    assert fn.argtypes == args and fn.restype is C.c_int


def test_plan_waves_rejects_bad_input():
    """KAO_ERR_INVALID (-1) for every malformed call, checked on the host before any device is used."""
    cur = np.array([[0, 1], [2, 3]])
    tgt = np.array([[0, 4], [2, 3]])
    assert _call(5, cur, tgt, 0) == -1                                    # k < 1
    assert _call(5, cur, tgt, 1, W=0) == -1 and _call(5, cur, tgt, 1, W=9) == -1  # width outside 1..8
    assert _call(0, cur, tgt, 1) == -1 and _call(65535, cur, tgt, 1) == -1        # n_brokers outside 1..65534
    assert _call(4, cur, tgt, 1) == -1                                    # broker 4 >= n_brokers
    assert _call(5, cur, np.array([[0, 0], [2, 3]]), 1) == -1             # broker repeated in a target row
    assert _call(5, np.array([[1, 1], [2, 3]]), tgt, 1) == -1             # ... in a current row
    assert _call(5, cur, np.array([[NONE, NONE], [2, 3]]), 1) == -1       # target row without a broker


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_plan_waves_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd import waves
    assert _call(5, np.array([[0, 1]]), np.array([[0, 4]]), 1) == -3   # KAO_ERR_NO_DEVICE
    with pytest.raises(kao.KaoError) as e:
        waves.plan_waves(load_golden("readme_current.json"), load_golden("readme_proposal.json"), 2)
    assert e.value.code == -3


def test_parse_pair_builds_the_union_broker_index():
    """Broker 19 leaves the cluster in the README example (--broker-list 0..18) but holds a replica of partition 1 today: it
    stays in the index, as a copy source."""
    from kafka_assignment_optimizer_amd.waves import parse_pair
    cur = load_golden("readme_current.json")
    plan = {"version": 1, "partitions": [{"topic": "x.y.z.t", "partition": 1, "replicas": [8, 1]}]}  # README.md:88
    wi = parse_pair(cur, plan)
    assert wi.broker_ids.tolist() == list(range(20))
    assert wi.keys == [("x.y.z.t", p) for p in range(10)]
    assert wi.current.shape == wi.target.shape == (10, 2)
    assert wi.current[1].tolist() == [8, 19] and wi.target[1].tolist() == [8, 1]
    # partitions the plan leaves out are unchanged
    others = [p for p in range(10) if p != 1]
    assert (wi.current[others] == wi.target[others]).all()
    # ids are mapped to dense indices (sorted union), not used as indices
    cur2 = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [1001, 7]},
                                         {"topic": "u", "partition": 3, "replicas": [7]}]}
    plan2 = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [7, 2000, 1001]}]}
    wi2 = parse_pair(cur2, plan2)
    assert wi2.broker_ids.tolist() == [7, 1001, 2000]
    assert wi2.current.tolist() == [[1, 0, NONE], [0, NONE, NONE]]
    assert wi2.target.tolist() == [[0, 2, 1], [0, NONE, NONE]]
    assert wi2.target_replicas == [[7, 2000, 1001], [7]]


def test_parse_pair_rejects_unknown_and_duplicate_partitions():
    from kafka_assignment_optimizer_amd.waves import parse_pair
    cur = load_golden("readme_current.json")
    with pytest.raises(ValueError, match="does not have"):
        parse_pair(cur, {"version": 1, "partitions": [{"topic": "x.y.z.t", "partition": 10, "replicas": [0, 1]}]})
    with pytest.raises(ValueError, match="does not have"):
        parse_pair(cur, {"version": 1, "partitions": [{"topic": "other", "partition": 1, "replicas": [0, 1]}]})
    dup = {"version": 1, "partitions": [{"topic": "x.y.z.t", "partition": 1, "replicas": [8, 1]}] * 2}
    with pytest.raises(ValueError, match="twice"):
        parse_pair(cur, dup)


def test_reference_checker_on_the_readme_proposal():
    """The test-side restatement on the README's proposal: all 10 partitions change and add brokers, the busiest brokers take
    part in 3 of them, so the lower bound is 3 / 2 / 1 for k = 1 / 2 / 3; the exact optimum of k = 1 is one wave more."""
    import waves_ref as wr
    from kafka_assignment_optimizer_amd.waves import parse_pair
    wi = parse_pair(load_golden("readme_current.json"), load_golden("readme_proposal.json"))
    cls, parts = wr.classify(wi.current, wi.target)
    assert cls == [1] * 10
    assert max(wr.degrees(parts).values()) == 3
    assert [wr.lower_bound(wi.current, wi.target, k) for k in (1, 2, 3)] == [3, 2, 1]
    assert [wr.ilp_min_waves(wi.current, wi.target, k) for k in (1, 2, 3)] == [4, 2, 1]


def test_cli_usage_errors():
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "cli", "kao-waves")
    assert subprocess.run([exe], capture_output=True).returncode == 2
    assert subprocess.run([exe, "--bogus"], capture_output=True).returncode == 2
    args = ["--plan", "p.json", "--out-prefix", "w", "--max-per-broker"]
    assert subprocess.run([exe, "--current", "c.json"] + args + ["0"], capture_output=True).returncode == 2
    r = subprocess.run([exe, "--current", "/nonexistent.json"] + args + ["1"], capture_output=True)
    assert r.returncode == 1 and b"cannot open" in r.stderr
