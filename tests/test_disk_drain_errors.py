"""kao_balance_disk_drain refuses bad input on the host, before any device is used: the shared refusals of
tests/test_disk_errors.py against the new symbol with the new prefix, the three new null pointers and a drain array that leaves no
live broker; the rows and the stats stay as they are.  The entry point is declared, exported and bound; both command-line tools refuse
--drain with the budget, capacity and exchange flags, an id outside --broker-list, a duplicate and every broker; the Python API refuses
the same before the library is loaded; without a device a valid call fails loudly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_disk_errors as shared
from conftest import ROOT, have_gpu

PREFIX = "kao_balance_disk_drain: "
ARGS = shared.ARGS[:7] + ("drain",) + shared.ARGS[7:17] + ("n_left", "bytes_left") + shared.ARGS[17:]


def _call(rows=((0, 1), (2, 3), (1, 2)), B=4, R=2, rack_of=None, size=(5, 6, 7), null=None, P=None, W=None, stats=True, drain=None):
    """(return code, kao_last_error()); asserts that the row buffer, the stats and the outputs are unchanged on error."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    rk = np.ascontiguousarray(np.arange(max(B, 1)) % max(R, 1) if rack_of is None else rack_of, dtype=np.uint8)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    dn = np.ascontiguousarray(np.arange(max(B, 1)) == 0 if drain is None else drain, dtype=np.uint8)   # broker 0 drains
    n, status, left = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    u = [C.c_uint64(77) for _ in range(5)]
    st = np.full(10, -7, dtype=np.int64)
    args = [B, R, rk.ctypes.data_as(C.POINTER(C.c_uint8)), r.shape[0] if P is None else P, r.shape[1] if W is None else W,
            r.ctypes.data_as(C.POINTER(C.c_uint16)), sz.ctypes.data_as(C.POINTER(C.c_uint64)), dn.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 1, 0, 0, 0, C.byref(n),
            C.byref(u[0]), C.byref(u[1]), C.byref(u[2]), C.byref(u[3]), C.byref(left), C.byref(u[4]), C.byref(status), st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[ARGS.index(null)] = None
    rc = lib.kao_balance_disk_drain(*args)
    if rc:   # a rejected call leaves the rows, the stats and every output alone
        assert (r == keep).all() and (st == -7).all() and (n.value, status.value, left.value) == (-7, -7, -7) and all(x.value == 77 for x in u)
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_disk_drain\(int32_t n_brokers, int32_t n_racks, const uint8_t \*rack_of, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/, const uint64_t \*size /\* \[n_partitions\] \*/,\s+"
                     r"const uint8_t \*drain /\* \[n_brokers\], != 0: this broker is to end empty \*/,\s+"
                     r"int32_t max_per_rack /\* <= 0: no rack rule \*/, int32_t move_leaders, uint64_t min_gain,\s+"
                     r"int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run, int32_t \*n_moved, uint64_t \*bytes_moved,\s+"
                     r"uint64_t \*peak_before, uint64_t \*peak_after, uint64_t \*lower_bound, int32_t \*n_left, uint64_t \*bytes_left,\s+"
                     r"int32_t \*status, int64_t stats\[10\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header   # no version bump, as for the earlier planners
    res, args = _ffi.SIGNATURES["kao_balance_disk_drain"]
    plain = _ffi.SIGNATURES["kao_balance_disk"][1]
    P = C.POINTER
    assert res is C.c_int and len(args) == len(ARGS) and args == plain[:7] + [P(C.c_uint8)] + plain[7:17] + [P(C.c_int32), P(C.c_uint64)] + plain[17:]
    bound = _ffi.load().kao_balance_disk_drain
    assert bound.argtypes == args and bound.restype is C.c_int


@pytest.mark.parametrize("what,change,code,text", shared.REFUSED, ids=[r[0] for r in shared.REFUSED])
def test_entry_point_refuses_what_the_plain_call_refuses(what, change, code, text):
    """The plain call's refusal with the new prefix, the same return code and the same text behind the prefix."""
    rc, msg = _call(**change)
    assert rc == code and msg.startswith(PREFIX) and text in msg, (rc, msg)
    assert shared._call(**change) == (code, "kao_balance_disk: " + msg[len(PREFIX):])


NEW_REFUSED = [
    ("null drain", dict(null="drain"), "null pointer"),
    ("null n_left", dict(null="n_left"), "null pointer"),
    ("null bytes_left", dict(null="bytes_left"), "null pointer"),
    ("every broker draining", dict(drain=[1, 1, 1, 1]), "no live broker"),
    ("every broker draining, any non-zero flag", dict(drain=[1, 255, 2, 7]), "no live broker"),
    ("the only broker draining", dict(rows=[[0], [0], [0]], B=1, R=1, drain=[1]), "no live broker"),
]


@pytest.mark.parametrize("what,change,text", NEW_REFUSED, ids=[r[0] for r in NEW_REFUSED])
def test_entry_point_refuses_the_new_cases(what, change, text):
    rc, msg = _call(**change)
    assert rc == shared.INVALID and msg.startswith(PREFIX) and text in msg, (rc, msg)


def test_the_shared_checks_come_before_the_count_of_live_brokers():
    """A bad row with every broker draining is the row's refusal: the checks of kao_balance_disk run first."""
    rc, msg = _call(rows=[[0, 1], [3, 3], [1, 2]], drain=[1, 1, 1, 1])
    assert rc == shared.INVALID and "partition 1" in msg


def test_valid_calls_pass_the_host_checks():
    """None is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    assert _call(stats=False)[0] == want and _call(stats=True)[0] == want
    assert _call(drain=[0, 0, 0, 0])[0] == want and _call(drain=[1, 1, 1, 0])[0] == want   # no draining broker; one live broker
    assert _call(rows=np.zeros((0, 2)), size=np.zeros(1), P=0)[0] == want              # no partition


BASE = ["--current", "none.json", "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--sizes", "none.txt", "--out", "none.out"]
FLAG_ERRORS = [(["--drain", "1", "--max-bytes", "1G"], "--drain works by bytes only"), (["--drain", "1", "--capacities", "0:1G,1:1G,2:1G"], "--drain works by bytes only"),
               (["--drain", "1", "--default-capacity", "1G"], "--drain works by bytes only"), (["--drain", "1", "--exchange"], "--drain works by bytes only"),
               (["--drain", "7"], "broker 7 is not in the broker list"), (["--drain", "1,1"], "broker 1 is named twice"), (["--drain", "0,2,1"], "every broker is draining"),
               (["--drain", "x"], "--drain needs broker ids"), (["--drain", ""], "--drain needs broker ids")]


@pytest.mark.parametrize("flags,text", FLAG_ERRORS, ids=["+".join(f[0]) for f in FLAG_ERRORS])
def test_both_tools_refuse(flags, text, capsys):
    """A usage error (exit status 2) with a message, before any file is read."""
    from kafka_assignment_optimizer_amd.disk import main
    with pytest.raises(SystemExit) as e:
        main(BASE + flags)
    assert e.value.code == 2 and text in capsys.readouterr().err
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-disk")] + BASE + flags, capture_output=True, cwd=ROOT)
    assert r.returncode == 2 and text.encode() in r.stderr, r.stderr


def test_both_tools_take_drain_alone_and_document_it(tmp_path):
    base = ["--current", str(tmp_path / "none.json"), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--sizes", str(tmp_path / "s.txt"), "--out",
            str(tmp_path / "o.json"), "--drain", "2,0", "--max-per-rack", "1", "--keep-leaders", "--min-gain", "1K", "--max-rounds", "3", "--dry-run", "--report"]
    for prog in ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"]):
        r = subprocess.run(prog + base, capture_output=True, cwd=ROOT)
        assert r.returncode == 1, (prog, r.stderr)   # past the usage checks: the missing document
        h = subprocess.run(prog + ["--help"], capture_output=True, cwd=ROOT)
        assert b"--drain" in h.stdout + h.stderr and b"3" in h.stdout + h.stderr
    usage = subprocess.run([os.path.join(ROOT, "cli", "kao-disk"), "--help"], capture_output=True, cwd=ROOT).stderr
    assert b"3 = with --drain, replicas are left" in usage


def test_python_api_refuses_before_the_library_is_loaded():
    from kafka_assignment_optimizer_amd.disk import DRAIN_STAT_KEYS, DiskResult, balance_disk, balance_disk_arrays, drain_flags
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    for kw in (dict(max_bytes=10), dict(capacity=[5, 5, 5]), dict(exchange=True), dict(max_bytes=0, capacity=[5, 5, 5])):
        with pytest.raises(ValueError, match="drain works by bytes only"):
            balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], drain=[1, 0, 0], **kw)
    with pytest.raises(ValueError, match="every broker is draining"):
        balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], drain=[1, 1, 1])
    with pytest.raises(ValueError, match="one flag per broker"):
        balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], drain=[1, 0])
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [0, 1]}]}
    for drain, text in (([5], "not in the broker list"), ([1, 1], "named twice"), ([0, 1], "every broker is draining")):
        with pytest.raises(ValueError, match=text):
            balance_disk(doc, {("t", 0): 5}, broker_list=[0, 1], racks={0: "a", 1: "a"}, drain=drain)
    with pytest.raises(ValueError, match="drain works by bytes only"):
        balance_disk(doc, {("t", 0): 5}, broker_list=[0, 1], racks={0: "a", 1: "a"}, drain=[1], max_bytes=1)
    assert drain_flags([10, 20, 30], [30, 10]).tolist() == [1, 0, 1]
    assert len(DRAIN_STAT_KEYS) == 10 and DRAIN_STAT_KEYS[8:] == ("drain_moves", "last_drain_round")
    assert {"drain", "n_left", "bytes_left", "drain_moves", "last_drain_round"} <= set(DiskResult.__dataclass_fields__)


def test_report_gains_the_drain_numbers_and_one_line_per_replica_left():
    from kafka_assignment_optimizer_amd.disk import DiskPlan, DiskResult, left_replicas, report_lines
    from kafka_assignment_optimizer_amd.failover import parse_current
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [10, 11]}, {"topic": "t", "partition": 1, "replicas": [10]}]}
    fi = parse_current(doc, [10, 11, 12], {10: "a", 11: "b", 12: "b"})
    kw = dict(rows=fi.rows, n_moved=3, bytes_moved=30, peak_before=9, peak_after=7, lower_bound=7, status="FEASIBLE_BOUND_GAP")
    size = np.array([5, 2], dtype=np.uint64)
    plain = report_lines(DiskPlan(DiskResult(stats=np.array([0, 1, 2, 3, 4, 5, 1, 7]), **kw), fi, size))
    drain = np.array([1, 0, 0], dtype=np.uint8)
    left = [("t", p, int(fi.broker_ids[fi.rows[p][j]]), why) for p, j, why in left_replicas(fi.rows, fi.rack_of, drain, 1)]
    assert left == [("t", 0, 10, "rack_rule"), ("t", 1, 10, "max_rounds")]   # row 0: rack b is at its cap; row 1: brokers 11 and 12 would take it
    assert [w for _, _, w in left_replicas(fi.rows, fi.rack_of, np.array([1, 0, 1]), 0)] == ["row_holds_every_live_broker", "max_rounds"]
    both = report_lines(DiskPlan(DiskResult(stats=np.array([0, 1, 2, 3, 4, 5, 1, 7, 8, 9]), drain=drain, n_left=2, bytes_left=7, drain_moves=8, last_drain_round=9, **kw), fi,
                                 size, left=left))
    assert len(plain) == 1 and both == [plain[0] + " draining=10 drain_bytes_before=7 drain_bytes_after=7 drain_moves=8 last_drain_round=9 replicas_left=2 bytes_left=7",
                                        "disk: left t-0 broker=10 reason=rack_rule", "disk: left t-1 broker=10 reason=max_rounds"]


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.disk import balance_disk_arrays
    with pytest.raises(kao.KaoError) as e:
        balance_disk_arrays(np.array([[0, 1], [0, 2], [1, 2]]), 3, [0, 0, 0], 1, [4, 5, 6], drain=[1, 0, 0])
    assert e.value.code == -3 and "kao_balance_disk_drain" in str(e.value)
