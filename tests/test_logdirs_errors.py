"""kao_balance_logdirs refuses bad input on the host, before any device is used: one case per refusal of
include/kao.h, each with its return code and a text in kao_last_error(); dir[] stays as it is.  The entry point is declared,
exported and bound, and without a device a valid call fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu

INVALID, UNSUPPORTED = -1, -2
ARGS = ("n_brokers", "dir_start", "base", "n_replicas", "dir", "size", "min_gain", "max_rounds", "dry_run", "n_moved", "bytes_moved", "peak_before",
        "peak_after", "per_broker", "status", "stats")


def _call(dir_start=(0, 2, 2, 5), base=(0, 7, 0, 0, 1), dir=(0, 0, 1, 4, 2), size=(5, 6, 7, 8, 9), null=None, B=None, R=None, stats=False):
    """(return code, kao_last_error()); asserts that the dir buffer is unchanged."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    ds = np.ascontiguousarray(dir_start, dtype=np.int32)
    d = np.ascontiguousarray(dir, dtype=np.int32)
    keep = d.copy()
    bs = None if base is None else np.ascontiguousarray(base, dtype=np.uint64)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    nb = len(ds) - 1 if B is None else B
    n, status = C.c_int32(0), C.c_int32(0)
    u = [C.c_uint64(0) for _ in range(3)]
    per = np.zeros(6 * max(min(nb, 70000), 1), dtype=np.uint64)
    st = np.zeros(8, dtype=np.int64)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    args = [nb, ds.ctypes.data_as(i32p), None if bs is None else bs.ctypes.data_as(u64p), d.shape[0] if R is None else R, d.ctypes.data_as(i32p),
            sz.ctypes.data_as(u64p), 0, 0, 0, C.byref(n), C.byref(u[0]), C.byref(u[1]), C.byref(u[2]), per.ctypes.data_as(u64p), C.byref(status),
            st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[ARGS.index(null)] = None
    rc = lib.kao_balance_logdirs(*args)
    assert (d == keep).all()   # a rejected call leaves dir[] alone
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_logdirs\(int32_t n_brokers, const int32_t \*dir_start /\* \[n_brokers\+1\] \*/, const uint64_t \*base /\* \[n_dirs\] or NULL \*/,\s+"
                     r"int32_t n_replicas, int32_t \*dir /\* \[n_replicas\] in / out \*/, const uint64_t \*size /\* \[n_replicas\] \*/,\s+"
                     r"uint64_t min_gain, int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run,\s+"
                     r"int32_t \*n_moved, uint64_t \*bytes_moved, uint64_t \*peak_before, uint64_t \*peak_after,\s+"
                     r"uint64_t \*per_broker /\* \[n_brokers\*6\] \*/, int32_t \*status, int64_t stats\[8\] /\* may be NULL \*/\);", header)
    assert re.search(r"#define KAO_LOGDIRS_MAX_DIRS 64\b", header) and "#define KAO_VERSION 103" in header   # no version bump, as for the earlier planners
    res, args = _ffi.SIGNATURES["kao_balance_logdirs"]
    P = C.POINTER
    assert res is C.c_int and len(args) == len(ARGS)
    assert args == [C.c_int32, P(C.c_int32), P(C.c_uint64), C.c_int32, P(C.c_int32), P(C.c_uint64), C.c_uint64, C.c_int32, C.c_int32, P(C.c_int32),
                    P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), P(C.c_int32), P(C.c_int64)]
    bound = _ffi.load().kao_balance_logdirs
    assert bound.argtypes == args and bound.restype is C.c_int


REFUSED = [
    ("null dir_start", dict(null="dir_start"), INVALID, "null pointer"),
    ("null dir", dict(null="dir"), INVALID, "null pointer"),
    ("null size", dict(null="size"), INVALID, "null pointer"),
    ("null n_moved", dict(null="n_moved"), INVALID, "null pointer"),
    ("null bytes_moved", dict(null="bytes_moved"), INVALID, "null pointer"),
    ("null peak_before", dict(null="peak_before"), INVALID, "null pointer"),
    ("null peak_after", dict(null="peak_after"), INVALID, "null pointer"),
    ("null per_broker", dict(null="per_broker"), INVALID, "null pointer"),
    ("null status", dict(null="status"), INVALID, "null pointer"),
    ("no broker", dict(B=0), INVALID, "n_brokers"),
    ("too many brokers", dict(B=65535), INVALID, "n_brokers"),
    ("dir_start[0] != 0", dict(dir_start=[1, 2, 2, 5]), INVALID, "dir_start[0]"),
    ("dir_start decreasing", dict(dir_start=[0, 3, 2, 5]), INVALID, "broker 1"),
    ("negative replicas", dict(R=-1), INVALID, "n_replicas"),
    ("dir[r] below 0", dict(dir=[0, 0, -1, 4, 2]), INVALID, "dir[2]"),
    ("dir[r] == n_dirs", dict(dir=[0, 0, 1, 5, 2]), INVALID, "dir[3]"),
    ("a replica and no dir at all", dict(dir_start=[0, 0], base=None, dir=[0], size=[1]), INVALID, "dir[0]"),
    ("sizes sum to 2^62", dict(size=[2 ** 61, 2 ** 61, 0, 0, 0], base=None), INVALID, "2^62"),
    ("sizes sum past 2^64", dict(size=[2 ** 63, 2 ** 63, 5, 0, 0]), INVALID, "2^62"),
    ("bases and sizes sum to 2^62", dict(base=[2 ** 61, 0, 0, 0, 2 ** 60], size=[2 ** 60, 0, 0, 0, 0]), INVALID, "2^62"),
    ("bases sum past 2^64", dict(base=[2 ** 63, 2 ** 63, 0, 0, 0]), INVALID, "2^62"),
    ("65 dirs on one broker", dict(dir_start=[0, 2, 67], base=None, dir=[0, 66], size=[1, 2]), UNSUPPORTED, "broker 1"),
    # one real replica behind a count that says more: the call returns before it reads a replica
    ("more than 4,000,000 replicas", dict(dir=[0], size=[1], R=4000001), UNSUPPORTED, "4,000,000"),
]


@pytest.mark.parametrize("what,change,code,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_entry_point_refuses(what, change, code, text):
    rc, msg = _call(**change)
    assert rc == code and msg.startswith("kao_balance_logdirs: ") and text in msg, (rc, msg)


def test_base_and_stats_may_be_null_and_limits_pass_the_host_checks():
    """None of these is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    assert _call(stats=False)[0] == want and _call(stats=True)[0] == want and _call(base=None)[0] == want
    assert _call(base=[2 ** 61 - 1, 0, 0, 0, 2 ** 60], size=[2 ** 60, 0, 0, 0, 0])[0] == want   # 2^62 - 1
    assert _call(dir_start=[0, 0, 64], base=None, dir=[63, 0], size=[1, 2])[0] == want          # KAO_LOGDIRS_MAX_DIRS dirs, a broker without one
    assert _call(dir_start=[0, 3], base=None, dir=[0], size=[0], R=0)[0] == want                # no replica


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays
    with pytest.raises(kao.KaoError) as e:
        balance_logdirs_arrays([0, 2], [0, 0, 1], [4, 5, 6])
    assert e.value.code == -3
    for bad in (dict(size=[4, 5]), dict(size=[4, -5, 6]), dict(size=[4.0, 5.0, 6.0]), dict(base=[1]), dict(min_gain=-1), dict(min_gain=2 ** 64)):
        with pytest.raises(ValueError):   # the binding's own checks come before the library
            balance_logdirs_arrays(**dict(dict(dir_start=[0, 2], dir=[0, 0, 1], size=[4, 5, 6]), **bad))


ARRAY_CHECKS = [   # in the order of the checks: a case with two faults gets the text of the earlier one
    (dict(exchange=True, capacity=[10, 10], dir_start=[0]), "exchange moves are by bytes only: exchange=True cannot be combined with capacity"),
    (dict(dir_start=[0], size=[4, 5]), "dir_start must hold n_brokers + 1 values, n_brokers >= 1"),
    (dict(dir_start=[]), "dir_start must hold n_brokers + 1 values, n_brokers >= 1"),
    (dict(size=[4, 5], min_gain=-1), "size must hold one value per replica (3), got 2"),
    (dict(size=[4, -5, 6], min_gain=-1), "sizes must be integers >= 0"),
    (dict(size=[4.0, 5.0, 6.0]), "sizes must be integers >= 0"),
    (dict(min_gain=-1, base=[1]), "min_gain must be 0..2^64-1"),
    (dict(min_gain=2 ** 64), "min_gain must be 0..2^64-1"),
    (dict(min_gain=True), "min_gain must be 0..2^64-1"),
    (dict(base=[1], capacity=[0, 0]), "base must hold one value per dir (2), got 1"),
    (dict(base=[1, -1]), "bases must be integers >= 0"),
    (dict(base=[1.0, 2.0]), "bases must be integers >= 0"),
    (dict(capacity=[10]), "capacity must hold one value per dir (2), got 1"),
]


@pytest.mark.parametrize("bad,text", ARRAY_CHECKS, ids=[f"{i}-{t[:24]}" for i, (_, t) in enumerate(ARRAY_CHECKS)])
def test_array_checks_refuse_with_their_texts(bad, text):
    """The checks of balance_logdirs_arrays before the library is called, with or without a device: the text, and the order of the checks."""
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays
    with pytest.raises(ValueError) as e:
        balance_logdirs_arrays(**dict(dict(dir_start=[0, 2], dir=[0, 0, 1], size=[4, 5, 6]), **bad))
    assert str(e.value) == text
