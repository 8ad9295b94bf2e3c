"""kao_balance_disk_capacity refuses bad input on the host, before any device is used: the refusals of
kao_balance_disk, each with its return code and a text in kao_last_error() that names this entry point, and its own for the
capacities; the rows stay as they are.  The entry point is declared, exported and bound, and without a device a valid call fails
loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu

NONE = 0xFFFF
INVALID, UNSUPPORTED = -1, -2
ARGS = ("n_brokers", "n_racks", "rack_of", "n_partitions", "width", "rows", "size", "cap", "max_per_rack", "move_leaders", "min_gain", "max_bytes",
        "max_rounds", "dry_run", "n_moved", "bytes_moved", "peak_before", "peak_after", "lower_bound", "status", "stats")
PREFIX = "kao_balance_disk_capacity: "


def _call(rows=((0, 1), (2, 3), (1, 2)), B=4, R=2, rack_of=None, size=(5, 6, 7), cap=None, null=None, P=None, W=None, stats=False, max_bytes=2 ** 64 - 1,
          dry_run=0):
    """(return code, kao_last_error()); asserts that the row buffer is unchanged (a valid call is made with dry_run: with a device it
    runs, and would move replicas)."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    rk = np.ascontiguousarray(np.arange(max(B, 1)) % max(R, 1) if rack_of is None else rack_of, dtype=np.uint8)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    cp = np.ascontiguousarray([1000 + b for b in range(max(B, 1))] if cap is None else cap, dtype=np.uint64)
    n, status, moved = C.c_int32(0), C.c_int32(0), C.c_uint64(0)
    u = [(C.c_uint64 * 2)() for _ in range(3)]
    st = np.zeros(11, dtype=np.int64)
    args = [B, R, rk.ctypes.data_as(C.POINTER(C.c_uint8)), r.shape[0] if P is None else P, r.shape[1] if W is None else W,
            r.ctypes.data_as(C.POINTER(C.c_uint16)), sz.ctypes.data_as(C.POINTER(C.c_uint64)), cp.ctypes.data_as(C.POINTER(C.c_uint64)), 0, 1, 0, max_bytes, 0,
            dry_run, C.byref(n), C.byref(moved), u[0], u[1], u[2], C.byref(status), st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[ARGS.index(null)] = None
    rc = lib.kao_balance_disk_capacity(*args)
    assert (r == keep).all()   # a rejected call leaves the rows alone
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_disk_capacity\(int32_t n_brokers, int32_t n_racks, const uint8_t \*rack_of, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/, const uint64_t \*size /\* \[n_partitions\] \*/,\s+"
                     r"const uint64_t \*cap /\* \[n_brokers\] \*/, int32_t max_per_rack /\* <= 0: no rack rule \*/,\s+"
                     r"int32_t move_leaders, uint64_t min_gain, uint64_t max_bytes /\* UINT64_MAX: no budget \*/,\s+"
                     r"int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run, int32_t \*n_moved, uint64_t \*bytes_moved,\s+"
                     r"uint64_t peak_before\[2\], uint64_t peak_after\[2\], uint64_t lower_bound\[2\], int32_t \*status,\s+"
                     r"int64_t stats\[11\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header   # no version bump, as for the earlier planners
    assert header.index("int kao_balance_disk_budget(") < header.index("int kao_balance_disk_capacity(")
    res, args = _ffi.SIGNATURES["kao_balance_disk_capacity"]
    assert res is C.c_int and len(args) == len(ARGS)
    budget = _ffi.SIGNATURES["kao_balance_disk_budget"][1]
    assert args[:7] + args[8:] == budget and args[7] == C.POINTER(C.c_uint64)   # kao_balance_disk_budget's arguments with cap after size
    bound = _ffi.load().kao_balance_disk_capacity
    assert bound.argtypes == args and bound.restype is C.c_int


REFUSED = [
    ("null rack_of", dict(null="rack_of"), INVALID, "null pointer"),
    ("null rows", dict(null="rows"), INVALID, "null pointer"),
    ("null size", dict(null="size"), INVALID, "null pointer"),
    ("null n_moved", dict(null="n_moved"), INVALID, "null pointer"),
    ("null bytes_moved", dict(null="bytes_moved"), INVALID, "null pointer"),
    ("null peak_before", dict(null="peak_before"), INVALID, "null pointer"),
    ("null peak_after", dict(null="peak_after"), INVALID, "null pointer"),
    ("null lower_bound", dict(null="lower_bound"), INVALID, "null pointer"),
    ("null status", dict(null="status"), INVALID, "null pointer"),
    ("width 0", dict(W=0), INVALID, "width"),
    ("width above KAO_MAX_RF", dict(W=9), INVALID, "width"),
    ("no broker", dict(B=0), INVALID, "n_brokers"),
    ("too many brokers", dict(B=65535), INVALID, "n_brokers"),
    ("no rack", dict(R=0), INVALID, "n_racks"),
    ("too many racks", dict(R=256), INVALID, "n_racks"),
    ("rack_of[b] >= n_racks", dict(rack_of=[0, 1, 2, 1]), INVALID, "rack_of[2]"),
    ("negative partitions", dict(P=-1), INVALID, "n_partitions"),
    ("slot 0 empty", dict(rows=[[0, 1], [NONE, 3], [1, 2]]), INVALID, "partition 1"),
    ("a broker after an empty slot", dict(rows=[[0, NONE, 1], [2, 3, NONE], [1, 2, 0]]), INVALID, "partition 0"),
    ("index >= n_brokers", dict(rows=[[0, 1], [2, 4], [1, 2]]), INVALID, "partition 1"),
    ("broker twice", dict(rows=[[0, 1], [3, 3], [1, 2]]), INVALID, "partition 1"),
    ("replica sizes sum to 2^62", dict(size=[2 ** 60, 2 ** 60, 0]), INVALID, "2^62"),
    ("replica sizes sum past 2^64", dict(size=[2 ** 63, 2 ** 63, 5]), INVALID, "2^62"),
    ("one size of 2^61 on two brokers", dict(size=[0, 0, 2 ** 61]), INVALID, "2^62"),
    # one real row behind a count that says more: the call returns before it reads a row
    ("more than 4,000,000 slots", dict(rows=[[0, 1]], size=[1], P=2000001), UNSUPPORTED, "4,000,000"),
    ("more than KAO_DISK_MAX_BROKERS brokers", dict(rows=[[0, 8000]], size=[1], B=8001, P=1 << 20), UNSUPPORTED, "8000"),
]
OWN = [
    ("null cap", dict(null="cap"), INVALID, "null pointer"),
    ("a capacity of 0", dict(cap=[5, 5, 0, 5]), INVALID, "cap[2] is 0"),
    ("capacities sum to 2^62", dict(cap=[2 ** 60] * 4), INVALID, "capacities sum to 2^62"),
    ("capacities sum past 2^64", dict(cap=[2 ** 63, 2 ** 63, 5, 5]), INVALID, "capacities sum to 2^62"),
    ("one capacity of 2^62", dict(cap=[1, 2 ** 62, 1, 1]), INVALID, "capacities sum to 2^62"),
]


@pytest.mark.parametrize("max_bytes", [0, 2 ** 64 - 1])
@pytest.mark.parametrize("what,change,code,text", REFUSED + OWN, ids=[r[0] for r in REFUSED + OWN])
def test_entry_point_refuses(what, change, code, text, max_bytes):
    rc, msg = _call(max_bytes=max_bytes, **change)
    assert rc == code and msg.startswith(PREFIX) and text in msg, (rc, msg)


def test_the_refusals_are_those_of_kao_balance_disk():
    """The same checks in the same order: the same code and, after the prefix, the same text; a bad capacity is reported after them."""
    import test_disk_errors as plain
    assert [r[:1] + r[2:] for r in REFUSED] == [r[:1] + r[2:] for r in plain.REFUSED]
    for what, change, _, _ in REFUSED:
        rc, msg = _call(**change)
        rc0, msg0 = plain._call(**change)
        assert rc == rc0 and msg.startswith(PREFIX) and msg0.startswith("kao_balance_disk: "), what
        assert msg[len(PREFIX):] == msg0[len("kao_balance_disk: "):], what
    rc, msg = _call(rows=[[0, 1], [3, 3], [1, 2]], cap=[5, 0, 5, 5])
    assert rc == INVALID and "partition 1" in msg


def test_stats_may_be_null_and_the_largest_capacities_pass_the_host_checks():
    """None is a refusal: every call gets as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    assert _call(stats=False, dry_run=1)[0] == want and _call(stats=True, dry_run=1)[0] == want
    assert _call(cap=[1, 1, 1, 1], dry_run=1)[0] == want
    assert _call(cap=[2 ** 60, 2 ** 60, 2 ** 60, 2 ** 60 - 1], dry_run=1)[0] == want   # the sum is 2^62 - 1
    for max_bytes in (0, 1, 2 ** 63, 2 ** 64 - 2, 2 ** 64 - 1):
        assert _call(max_bytes=max_bytes, dry_run=1)[0] == want, max_bytes


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.disk import balance_disk_arrays
    with pytest.raises(kao.KaoError) as e:
        balance_disk_arrays(np.array([[0, 1], [0, 2], [1, 2]]), 3, [0, 0, 0], 1, [4, 5, 6], capacity=[10, 20, 30])
    assert e.value.code == -3
