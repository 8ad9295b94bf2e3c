"""kao_balance_logdirs_exchange refuses bad input on the host, before any device is used: the shared cases of
tests/test_logdirs_errors.py, each with its return code and a text in kao_last_error(); dir[] stays as it is.  The entry point and
its test hook are declared, exported and bound, the binding refuses exchange together with capacities, and without a device a valid
call fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_logdirs_errors as shared
from conftest import ROOT, have_gpu

ARGS = shared.ARGS


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
    per = np.zeros(8 * max(min(nb, 70000), 1), dtype=np.uint64)
    st = np.zeros(12, dtype=np.int64)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    args = [nb, ds.ctypes.data_as(i32p), None if bs is None else bs.ctypes.data_as(u64p), d.shape[0] if R is None else R, d.ctypes.data_as(i32p),
            sz.ctypes.data_as(u64p), 0, 0, 0, C.byref(n), C.byref(u[0]), C.byref(u[1]), C.byref(u[2]), per.ctypes.data_as(u64p), C.byref(status),
            st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[ARGS.index(null)] = None
    rc = lib.kao_balance_logdirs_exchange(*args)
    assert (d == keep).all()   # a rejected call leaves dir[] alone
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_logdirs_exchange\(int32_t n_brokers, const int32_t \*dir_start /\* \[n_brokers\+1\] \*/, const uint64_t \*base /\* \[n_dirs\] or NULL \*/,\s+"
                     r"int32_t n_replicas, int32_t \*dir /\* \[n_replicas\] in / out \*/, const uint64_t \*size /\* \[n_replicas\] \*/,\s+"
                     r"uint64_t min_gain, int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run,\s+"
                     r"int32_t \*n_moved, uint64_t \*bytes_moved, uint64_t \*peak_before, uint64_t \*peak_after,\s+"
                     r"uint64_t \*per_broker /\* \[n_brokers\*8\] \*/, int32_t \*status, int64_t stats\[12\] /\* may be NULL \*/\);", header)
    assert re.search(r"\bint kao_logdirs_test_exchange\(int32_t path\);", header) and "#define KAO_VERSION 103" in header
    res, args = _ffi.SIGNATURES["kao_balance_logdirs_exchange"]
    assert res is C.c_int and args == _ffi.SIGNATURES["kao_balance_logdirs"][1] and len(args) == len(ARGS)
    lib = _ffi.load()
    assert lib.kao_balance_logdirs_exchange.argtypes == args and lib.kao_balance_logdirs_exchange.restype is C.c_int
    assert _ffi.SIGNATURES["kao_logdirs_test_exchange"] == (C.c_int, [C.c_int32])


def test_the_path_hook_returns_the_previous_choice_and_refuses_others():
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    assert lib.kao_logdirs_test_exchange(2) == 0 and lib.kao_logdirs_test_exchange(1) == 2 and lib.kao_logdirs_test_exchange(0) == 1
    for bad in (-1, 3):
        assert lib.kao_logdirs_test_exchange(bad) == shared.INVALID and "kao_logdirs_test_exchange" in lib.kao_last_error().decode()
    assert lib.kao_logdirs_test_exchange(0) == 0


@pytest.mark.parametrize("what,change,code,text", shared.REFUSED, ids=[r[0] for r in shared.REFUSED])
def test_entry_point_refuses(what, change, code, text):
    rc, msg = _call(**change)
    assert rc == code and msg.startswith("kao_balance_logdirs_exchange: ") and text in msg, (rc, msg)


def test_base_and_stats_may_be_null_and_limits_pass_the_host_checks():
    """None of these is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    assert _call(stats=False)[0] == want and _call(stats=True)[0] == want and _call(base=None)[0] == want
    assert _call(base=[2 ** 61 - 1, 0, 0, 0, 2 ** 60], size=[2 ** 60, 0, 0, 0, 0])[0] == want   # 2^62 - 1
    assert _call(dir_start=[0, 0, 64], base=None, dir=[63, 0], size=[1, 2])[0] == want          # KAO_LOGDIRS_MAX_DIRS dirs, a broker without one
    assert _call(dir_start=[0, 3], base=None, dir=[0], size=[0], R=0)[0] == want                # no replica


def test_binding_refuses_exchange_with_capacities():
    """Before the library is called: a ValueError with a clear text, from the arrays call and from the documents call."""
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs, balance_logdirs_arrays
    with pytest.raises(ValueError, match="exchange.*bytes only"):
        balance_logdirs_arrays([0, 2], [0, 0, 1], [4, 5, 6], capacity=[10, 10], exchange=True)
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [1]}]}
    dirs = {"version": 1, "brokers": [{"broker": 1, "logDirs": [{"logDir": "/a", "error": None, "partitions": [{"partition": "t-0", "size": 5, "offsetLag": 0, "isFuture": False}]},
                                                                 {"logDir": "/b", "error": None, "partitions": []}]}]}
    for kw in (dict(default_capacity=100), dict(capacity={1: 100}), dict(use_total_bytes=True)):
        with pytest.raises(ValueError, match="exchange.*bytes only"):
            balance_logdirs(doc, dirs, exchange=True, **kw)


@pytest.mark.parametrize("flags", [["--utilisation"], ["--capacities", "caps.json"], ["--default-capacity", "1G"], ["--plan", "plan.json"], ["--evacuate", "1:/a"],
                                   ["--plan", "plan.json", "--rebalance"]], ids=lambda f: f[0] + ("+rebalance" if len(f) > 2 else ""))
def test_python_cli_refuses_exchange_with_the_other_modes(flags, capsys):
    """A usage error (exit status 2) with a message, before any file is read."""
    from kafka_assignment_optimizer_amd.logdirs import main
    with pytest.raises(SystemExit) as e:
        main(["--current", "none.json", "--log-dirs", "none.txt", "--out", "none.out", "--exchange"] + flags)
    assert e.value.code == 2 and "--exchange cannot be combined" in capsys.readouterr().err


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays
    with pytest.raises(kao.KaoError) as e:
        balance_logdirs_arrays([0, 2], [0, 0, 1], [4, 5, 6], exchange=True)
    assert e.value.code == -3
