"""CPU tests of the failover-aware follower order (kao_failover_order): the HiGHS reference of
tests/failover_ref.py against enumeration on tiny instances, and the host restatement of the kernels' probes against both; the
composition of the small family the GPU test runs; the entry point is declared, exported and bound, rejects bad input before touching
a device and fails loudly without one; the Python front end's argument checks; the command-line tool's usage and input errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import failover_ref as fr
from conftest import ROOT, have_gpu

NONE = 0xFFFF


def test_reference_matches_enumeration_on_tiny_instances():
    family = fr.tiny_family()
    assert len(family) == 100
    improved = 0
    for i, (rows, B, rack_of, R) in enumerate(family):
        for scope in (0, 1):
            opt = fr.scenario_optimum(rows, B, rack_of, scope, R)
            assert opt[:, 0].max() <= 7
            assert (opt == fr.brute_force(rows, B, rack_of, scope, R)).all(), (i, scope)
            after, model = fr.kernel_model(rows, B, rack_of, scope, R)
            assert (model == opt).all(), (i, scope)
            assert fr.check_rows(rows, after, B, rack_of, scope) == opt[:, 4].sum()
            assert (fr.simulate(after, B, rack_of, scope, R) == opt[:, [0, 1, 3]]).all()
            improved += int((opt[:, 3] < opt[:, 2]).sum())
    assert improved >= 50, improved


def test_small_family_has_every_kind_of_scenario():
    """The composition the GPU test relies on, from the reference alone."""
    c = fr.composition(fr.small_family(), fr.small_family_optima())
    print(c)
    for kind, floor in fr.COMPOSITION_FLOORS.items():
        assert c[kind] >= floor, (kind, c)


def test_two_arc_instance_needs_a_path_of_two_arcs():
    rows, B, rack_of, R = fr.two_arc_instance()
    opt = fr.scenario_optimum(rows, B, rack_of, 0, R)
    assert opt[0].tolist() == [3, 0, 3, 2, 2]
    after, model = fr.kernel_model(rows, B, rack_of, 0, R)
    assert (model == opt).all() and after[0].tolist() == [0, 2, 1] and after[1].tolist() == [0, 3, 2]


def _call(B, R, rack_of, rows, scope=0, dry_run=0, null=None, P=None, W=None):
    from kafka_assignment_optimizer_amd import _ffi
    rows = np.ascontiguousarray(rows, dtype=np.uint16)
    rk = np.ascontiguousarray(rack_of, dtype=np.uint8)
    scen = np.zeros((max(B, R, 1), 5), dtype=np.int32)
    n = C.c_int32(0)
    args = [B, R, rk.ctypes.data_as(C.POINTER(C.c_uint8)), rows.shape[0] if P is None else P, rows.shape[1] if W is None else W,
            rows.ctypes.data_as(C.POINTER(C.c_uint16)), scope, dry_run, scen.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n), None]
    if null is not None:
        args[null] = None
    return _ffi.load().kao_failover_order(*args)


def test_failover_order_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_failover_order\(int32_t n_brokers, int32_t n_racks, const uint8_t \*rack_of /\* \[n_brokers\] \*/,\s+"
                     r"int32_t n_partitions, int32_t width, uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/,\s+"
                     r"int32_t scope /\* [^*]* \*/, int32_t dry_run,\s+"
                     r"int32_t \*scen /\* \[n_scen\*5\] \*/, int32_t \*n_reordered, int32_t stats\[8\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header
    assert int(re.search(r"#define KAO_FAILOVER_MAX_BROKERS (\d+)", header).group(1)) >= 4000
    res, args = _ffi.SIGNATURES["kao_failover_order"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [C.c_int32, C.c_int32, P(C.c_uint8), C.c_int32, C.c_int32, P(C.c_uint16), C.c_int32, C.c_int32, P(C.c_int32),
                    P(C.c_int32), P(C.c_int32)]
    fn = _ffi.load().kao_failover_order
    assert fn.argtypes == args and fn.restype is C.c_int


def _limit():
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    return int(re.search(r"#define KAO_FAILOVER_MAX_BROKERS (\d+)", header).group(1))


def test_failover_order_rejects_bad_input():
    """KAO_ERR_INVALID (-1) / KAO_ERR_UNSUPPORTED (-2) for every malformed call, checked on the host before any device is used."""
    rows = np.array([[0, 1, 2], [2, 3, NONE], [1, NONE, NONE]])
    rk = np.array([0, 1, 0, 1])
    for null in (2, 5, 8, 9):                                              # rack_of, rows, scen, n_reordered
        assert _call(4, 2, rk, rows, null=null) == -1
    for scope in (-1, 2):
        assert _call(4, 2, rk, rows, scope=scope) == -1
    for W in (0, 9):
        assert _call(4, 2, rk, rows, W=W) == -1
    for B in (0, 65535):
        assert _call(B, 2, np.zeros(max(B, 1)), rows) == -1
    for R in (0, 256):
        assert _call(4, R, rk, rows) == -1
    assert _call(4, 1, rk, rows) == -1                                     # rack_of[b] >= n_racks
    assert _call(4, 2, rk, np.array([[NONE, 1, 2]])) == -1                 # slot 0 not a broker
    assert _call(4, 2, rk, np.array([[0, NONE, 2]])) == -1                 # a broker after an empty slot
    assert _call(4, 2, rk, np.array([[0, 1, 4]])) == -1                    # index >= n_brokers
    assert _call(4, 2, rk, np.array([[0, 1, 0]])) == -1                    # broker twice in a row
    assert _call(4, 2, rk, rows, P=-1) == -1
    assert _call(4, 2, rk, rows, P=2000001, W=2) == -2                     # more than 4,000,000 slots, before a row is read
    lim = _limit()
    assert _call(lim + 1, 2, np.zeros(lim + 1), rows) == -2                # more brokers than a workgroup's LDS holds


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_failover_order_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.failover import failover_order_arrays
    rows = np.array([[0, 1, 2], [2, 3, NONE], [1, NONE, NONE]])
    rk = np.array([0, 1, 0, 1])
    assert _call(4, 2, rk, rows) == -3   # KAO_ERR_NO_DEVICE
    assert _call(_limit(), 2, np.zeros(_limit()), rows) == -3
    with pytest.raises(kao.KaoError) as e:
        failover_order_arrays(rows, 4, rk, 2, "rack")
    assert e.value.code == -3


def test_python_front_end_checks_its_arguments():
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd import failover as fo
    rows = np.array([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="scope"):
        fo.failover_order_arrays(rows, 3, np.zeros(3), 1, "zone")
    with pytest.raises(ValueError, match="width"):
        fo.failover_order_arrays(rows.reshape(-1), 3, np.zeros(3), 1, 0)
    with pytest.raises(ValueError, match="rack_of"):
        fo.failover_order_arrays(rows, 3, np.zeros(2), 1, 0)
    with pytest.raises(ValueError, match="broker_list"):
        fo.failover_order({"partitions": []}, "broker")
    with pytest.raises(ValueError, match="no topic"):
        fo.failover_order([], "broker")
    a = Topic(name="a", broker_ids=np.arange(3), rack_of=np.zeros(3), n_racks=1, n_partitions=2, rf=2, current=rows)
    b = Topic(name="b", broker_ids=np.arange(4), rack_of=np.zeros(4), n_racks=1, n_partitions=2, rf=2, current=rows)
    with pytest.raises(ValueError, match="one broker index"):
        fo.failover_order([a, b], "broker")
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 1, "replicas": [7, 5, 6]}, {"topic": "t", "partition": 0, "replicas": [5]},
                                        {"topic": "s", "partition": 3, "replicas": [6, 7]}]}
    fi = fo.parse_current(doc, [5, 6, 7], {5: "x", 6: "y", 7: "x"})
    assert fi.keys == [("s", 3), ("t", 0), ("t", 1)] and fi.rack_names == ["x", "y"] and fi.rack_of.tolist() == [0, 1, 0]
    assert fi.rows.tolist() == [[1, 2, NONE], [0, NONE, NONE], [2, 0, 1]]
    with pytest.raises(ValueError, match="outside --broker-list"):
        fo.parse_current(doc, [5, 6], {5: "x", 6: "y"})
    with pytest.raises(ValueError, match="no rack"):
        fo.parse_current(doc, [5, 6, 7], {5: "x", 6: "y"})


def test_cli_usage_and_input_errors(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "cli", "kao-failover")
    assert subprocess.run([exe], capture_output=True).returncode == 2
    assert subprocess.run([exe, "--bogus"], capture_output=True).returncode == 2
    base = ["--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a"]
    assert subprocess.run([exe, "--current", "c.json"] + base, capture_output=True).returncode == 2                      # no --scope
    assert subprocess.run([exe, "--current", "c.json", "--scope", "zone"] + base, capture_output=True).returncode == 2
    r = subprocess.run([exe, "--current", "/nonexistent.json", "--scope", "rack"] + base, capture_output=True)
    assert r.returncode == 1 and b"cannot open" in r.stderr
    cur = tmp_path / "cur.json"
    cur.write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"replicas":[0,1]},{"topic":"a","partition":7,"replicas":[2,5]}]}')
    r = subprocess.run([exe, "--current", str(cur), "--scope", "broker"] + base, capture_output=True)   # broker 5 is outside the list
    assert r.returncode == 1 and b"a-7" in r.stderr and b"--broker-list" in r.stderr
    from kafka_assignment_optimizer_amd.failover import main
    with pytest.raises(SystemExit) as e:
        main(["--current", str(cur), "--scope", "zone"] + base)
    assert e.value.code == 2
    assert main(["--current", str(cur), "--scope", "broker"] + base) == 1
    assert main(["--current", "/nonexistent.json", "--scope", "rack"] + base) == 1
