"""kao_place_logdirs refuses bad input on the host, before any device is used: one case per refusal of
include/kao.h, each with its return code and a text in kao_last_error(); dir[] stays as it is.  The entry point and the sort hook
are declared, exported and bound, and without a device a valid call fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, have_gpu

INVALID, UNSUPPORTED = -1, -2
ARGS = ("n_brokers", "dir_start", "base", "n_replicas", "broker", "dir", "size", "move_residents", "min_gain", "max_rounds", "dry_run", "n_placed",
        "bytes_placed", "n_moved", "bytes_moved", "peak_before", "peak_after", "per_broker", "status", "stats")


def _call(dir_start=(0, 2, 2, 5), base=(0, 7, 0, 0, 1), broker=(0, 0, 0, 2, 2), dir=(0, -1, 1, 4, -1), size=(5, 6, 7, 8, 9), null=None, B=None, R=None,
          stats=False, move_residents=0):
    """(return code, kao_last_error()); asserts that the dir buffer is unchanged."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    ds = np.ascontiguousarray(dir_start, dtype=np.int32)
    br = np.ascontiguousarray(broker, dtype=np.int32)
    d = np.ascontiguousarray(dir, dtype=np.int32)
    keep = d.copy()
    bs = None if base is None else np.ascontiguousarray(base, dtype=np.uint64)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    nb = len(ds) - 1 if B is None else B
    n = [C.c_int32(0) for _ in range(3)]
    u = [C.c_uint64(0) for _ in range(4)]
    per = np.zeros(8 * max(min(nb, 70000), 1), dtype=np.uint64)
    st = np.zeros(10, dtype=np.int64)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    args = [nb, ds.ctypes.data_as(i32p), None if bs is None else bs.ctypes.data_as(u64p), d.shape[0] if R is None else R, br.ctypes.data_as(i32p),
            d.ctypes.data_as(i32p), sz.ctypes.data_as(u64p), move_residents, 0, 0, 0, C.byref(n[0]), C.byref(u[0]), C.byref(n[1]), C.byref(u[1]), C.byref(u[2]),
            C.byref(u[3]), per.ctypes.data_as(u64p), C.byref(n[2]), st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[ARGS.index(null)] = None
    rc = lib.kao_place_logdirs(*args)
    if rc:
        assert (d == keep).all()   # a rejected call leaves dir[] alone
    return rc, lib.kao_last_error().decode()


def test_entry_point_and_hook_are_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_place_logdirs\(int32_t n_brokers, const int32_t \*dir_start /\* \[n_brokers\+1\] \*/, const uint64_t \*base /\* \[n_dirs\] or NULL \*/,\s+"
                     r"int32_t n_replicas, const int32_t \*broker /\* \[n_replicas\] \*/, int32_t \*dir /\* \[n_replicas\] in / out, -1 = homeless \*/,\s+"
                     r"const uint64_t \*size /\* \[n_replicas\] \*/, int32_t move_residents, uint64_t min_gain, int32_t max_rounds /\* <= 0: no limit \*/,\s+"
                     r"int32_t dry_run, int32_t \*n_placed, uint64_t \*bytes_placed, int32_t \*n_moved, uint64_t \*bytes_moved,\s+"
                     r"uint64_t \*peak_before, uint64_t \*peak_after, uint64_t \*per_broker /\* \[n_brokers\*8\] \*/, int32_t \*status,\s+"
                     r"int64_t stats\[10\] /\* may be NULL \*/\);", header)
    assert re.search(r"\bint kao_logdirs_test_sort\(int32_t path\);", header)
    assert "#define KAO_VERSION 103" in header   # no version bump, as for the earlier planners
    res, args = _ffi.SIGNATURES["kao_place_logdirs"]
    P = C.POINTER
    assert res is C.c_int and len(args) == len(ARGS)
    assert args == [C.c_int32, P(C.c_int32), P(C.c_uint64), C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_uint64), C.c_int32, C.c_uint64, C.c_int32, C.c_int32,
                    P(C.c_int32), P(C.c_uint64), P(C.c_int32), P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), P(C.c_int32), P(C.c_int64)]
    lib = _ffi.load()
    assert lib.kao_place_logdirs.argtypes == args and lib.kao_place_logdirs.restype is C.c_int
    assert _ffi.SIGNATURES["kao_logdirs_test_sort"] == (C.c_int, [C.c_int32])
    assert lib.kao_logdirs_test_sort.argtypes == [C.c_int32] and lib.kao_logdirs_test_sort.restype is C.c_int


def test_the_hook_sets_this_threads_choice_and_returns_the_previous_one():
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    assert lib.kao_logdirs_test_sort(3) == INVALID and "kao_logdirs_test_sort" in lib.kao_last_error().decode() and lib.kao_logdirs_test_sort(-1) == INVALID
    assert lib.kao_logdirs_test_sort(2) == 0 and lib.kao_logdirs_test_sort(1) == 2 and lib.kao_logdirs_test_sort(0) == 1 and lib.kao_logdirs_test_sort(0) == 0


REFUSED = [
    ("null dir_start", dict(null="dir_start"), INVALID, "null pointer"),
    ("null broker", dict(null="broker"), INVALID, "null pointer"),
    ("null dir", dict(null="dir"), INVALID, "null pointer"),
    ("null size", dict(null="size"), INVALID, "null pointer"),
    ("null n_placed", dict(null="n_placed"), INVALID, "null pointer"),
    ("null bytes_placed", dict(null="bytes_placed"), INVALID, "null pointer"),
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
    ("broker[r] below 0", dict(broker=[0, 0, -1, 2, 2]), INVALID, "broker[2]"),
    ("broker[r] == n_brokers", dict(broker=[0, 0, 0, 3, 2]), INVALID, "broker[3]"),
    ("dir[r] below -1", dict(dir=[0, -1, -2, 4, -1]), INVALID, "dir[2]"),
    ("dir[r] == n_dirs", dict(dir=[0, -1, 1, 5, -1]), INVALID, "dir[3]"),
    ("a resident in another broker's dir", dict(dir=[0, -1, 2, 4, -1]), INVALID, "dir[2] is not a dir of broker 0"),
    ("a resident on a broker without dirs", dict(broker=[0, 0, 1, 2, 2]), INVALID, "dir[2] is not a dir of broker 1"),
    ("a homeless replica on a broker without dirs", dict(broker=[0, 1, 0, 2, 2]), INVALID, "replica 1 is homeless on broker 1"),
    ("sizes sum to 2^62", dict(size=[2 ** 61, 2 ** 61, 0, 0, 0], base=None), INVALID, "2^62"),
    ("sizes sum past 2^64", dict(size=[2 ** 63, 2 ** 63, 5, 0, 0]), INVALID, "2^62"),
    ("bases and sizes sum to 2^62", dict(base=[2 ** 61, 0, 0, 0, 2 ** 60], size=[2 ** 60, 0, 0, 0, 0]), INVALID, "2^62"),
    ("bases sum past 2^64", dict(base=[2 ** 63, 2 ** 63, 0, 0, 0]), INVALID, "2^62"),
    ("65 dirs on one broker", dict(dir_start=[0, 2, 67], base=None, broker=[0, 1], dir=[0, -1], size=[1, 2]), UNSUPPORTED, "broker 1"),
    # one real replica behind a count that says more: the call returns before it reads a replica
    ("more than 4,000,000 replicas", dict(broker=[0], dir=[-1], size=[1], R=4000001), UNSUPPORTED, "4,000,000"),
]


@pytest.mark.parametrize("move_residents", [0, 1])
@pytest.mark.parametrize("what,change,code,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_entry_point_refuses(what, change, code, text, move_residents):
    rc, msg = _call(move_residents=move_residents, **change)
    assert rc == code and msg.startswith("kao_place_logdirs: ") and text in msg, (rc, msg)


def test_base_and_stats_may_be_null_and_limits_pass_the_host_checks():
    """None of these is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    assert _call(stats=False)[0] == want and _call(stats=True)[0] == want and _call(base=None)[0] == want and _call(move_residents=1)[0] == want
    assert _call(base=[2 ** 61 - 1, 0, 0, 0, 2 ** 60], size=[2 ** 60, 0, 0, 0, 0])[0] == want                     # 2^62 - 1
    assert _call(dir_start=[0, 0, 64], base=None, broker=[1, 1], dir=[63, -1], size=[1, 2])[0] == want           # KAO_LOGDIRS_MAX_DIRS dirs, a broker without one
    assert _call(dir_start=[0, 3], base=None, broker=[0], dir=[0], size=[0], R=0)[0] == want                     # no replica
    assert _call(dir=[-1, -1, -1, -1, -1])[0] == want and _call(dir=[0, 1, 1, 4, 2])[0] == want                  # all homeless, none homeless


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.logdirs import place_logdirs_arrays
    with pytest.raises(kao.KaoError) as e:
        place_logdirs_arrays([0, 2], [0, 0, 0], [0, -1, 1], [4, 5, 6])
    assert e.value.code == -3
    for bad in (dict(size=[4, 5]), dict(size=[4, -5, 6]), dict(size=[4.0, 5.0, 6.0]), dict(base=[1]), dict(min_gain=-1), dict(min_gain=2 ** 64),
                dict(broker=[0, 0]), dict(broker=[0.0, 0.0, 0.0])):
        with pytest.raises(ValueError):   # the binding's own checks come before the library
            place_logdirs_arrays(**dict(dict(dir_start=[0, 2], broker=[0, 0, 0], dir=[0, -1, 1], size=[4, 5, 6]), **bad))


ARRAY_CHECKS = [   # in the order of the checks: a case with two faults gets the text of the earlier one
    (dict(dir_start=[0], broker=[0, 0]), "dir_start must hold n_brokers + 1 values, n_brokers >= 1"),
    (dict(broker=[0, 0], size=[4, 5]), "broker must hold one value per replica (3), got 2"),
    (dict(broker=[0.0, 0.0, 0.0], size=[4, 5]), "brokers must be integers"),
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
    """The checks of place_logdirs_arrays before the library is called, with or without a device: the text, and the order of the checks."""
    from kafka_assignment_optimizer_amd.logdirs import place_logdirs_arrays
    with pytest.raises(ValueError) as e:
        place_logdirs_arrays(**dict(dict(dir_start=[0, 2], broker=[0, 0, 0], dir=[0, -1, 1], size=[4, 5, 6]), **bad))
    assert str(e.value) == text
