"""kao_balance_leaders_weighted_exchange refuses bad input on the host, before any device is used: the shared
invalid-argument cases of tests/test_wleaders_ref.py against the new symbol, each with KAO_ERR_INVALID and the new prefix in
kao_last_error(); the rows stay as they are.  The entry point is declared, exported and bound, both command-line tools refuse
--exchange without --traffic / --sizes and together with the unweighted flags, and without a device a valid call fails loudly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_wleaders_ref as shared
from conftest import ROOT, have_gpu

PREFIX = "kao_balance_leaders_weighted_exchange: "


def _call(rows, B, weight, min_gain=0, max_rounds=0, null=None, P=None, W=None, stats=True):
    """(return code, kao_last_error()); asserts that the row buffer is unchanged."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    wt = np.ascontiguousarray(weight, dtype=np.uint64)
    n, status = C.c_int32(0), C.c_int32(0)
    u = [C.c_uint64(0) for _ in range(3)]
    st = np.full(12, -7, dtype=np.int64)
    args = [B, r.shape[0] if P is None else P, r.shape[1] if W is None else W, r.ctypes.data_as(C.POINTER(C.c_uint16)),
            wt.ctypes.data_as(C.POINTER(C.c_uint64)), min_gain, max_rounds, 0, C.byref(n), C.byref(u[0]), C.byref(u[1]), C.byref(u[2]),
            C.byref(status), st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[null] = None
    rc = lib.kao_balance_leaders_weighted_exchange(*args)
    assert (r == keep).all()   # a rejected call leaves the rows alone
    if rc:
        assert (st == -7).all()
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_leaders_weighted_exchange\(int32_t n_brokers, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/, const uint64_t \*weight /\* \[n_partitions\] \*/,\s+"
                     r"uint64_t min_gain, int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run,\s+"
                     r"int32_t \*n_changed, uint64_t \*peak_before, uint64_t \*peak_after, uint64_t \*lower_bound,\s+"
                     r"int32_t \*status, int64_t stats\[12\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header and re.search(r"\bint64_t kao_wleaders_last_setup_us\(void\);", header)
    res, args = _ffi.SIGNATURES["kao_balance_leaders_weighted_exchange"]
    assert res is C.c_int and args == _ffi.SIGNATURES["kao_balance_leaders_weighted"][1] and len(args) == 14
    lib = _ffi.load()
    assert lib.kao_balance_leaders_weighted_exchange.argtypes == args and lib.kao_balance_leaders_weighted_exchange.restype is C.c_int
    assert _ffi.SIGNATURES["kao_wleaders_last_setup_us"] == (C.c_int64, []) and lib.kao_wleaders_last_setup_us() >= 0


@pytest.mark.parametrize("what,change", shared.INVALID, ids=[w for w, _ in shared.INVALID])
def test_entry_point_rejects_bad_input(what, change):
    """KAO_ERR_INVALID (-1) with the new prefix, checked on the host before any device is used; the rows and stats stay as they are.
    The text behind the prefix is the plain call's."""
    kw = dict(rows=[[0, 1], [2, 3], [1, 2]], B=4, weight=[5, 6, 7])
    kw.update(change)
    rc, msg = _call(**kw)
    assert rc == -1 and msg.startswith(PREFIX) and len(msg) > len(PREFIX), (rc, msg)
    from kafka_assignment_optimizer_amd import _ffi
    assert shared._call(**kw) == -1
    plain = _ffi.load().kao_last_error().decode()
    assert plain == "kao_balance_leaders_weighted: " + msg[len(PREFIX):]


def test_entry_point_reports_unsupported_sizes():
    rc, msg = _call(np.zeros((1, 2), dtype=np.uint16), 4, [1], P=2000001)   # more than 4,000,000 slots, before a row is read
    assert rc == -2 and msg.startswith(PREFIX)


def test_stats_may_be_null_and_limits_pass_the_host_checks():
    """None of these is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    assert _call(rows, 3, [4, 5, 6])[0] == want and _call(rows, 3, [4, 5, 6], stats=False)[0] == want
    assert _call(rows, 3, [2 ** 61 - 1, 2 ** 61, 0])[0] == want            # just below 2^62
    assert _call(rows, 3, [4, 5, 6], min_gain=2 ** 64 - 1, max_rounds=-3)[0] == want
    assert _call(np.zeros((0, 3)), 4, np.zeros(1), P=0)[0] == want          # no partition


FLAG_ERRORS = [["--exchange"], ["--exchange", "--cluster"], ["--exchange", "--slack", "1"], ["--exchange", "--auto-slack"], ["--exchange", "--cluster-hi", "4"],
               ["--exchange", "--traffic", "t.json", "--cluster"], ["--exchange", "--sizes", "s.txt", "--slack", "1"],
               ["--exchange", "--traffic", "t.json", "--sizes", "s.txt"], ["--exchange", "--traffic", "t.json", "--cluster-lo", "1"]]


@pytest.mark.parametrize("flags", FLAG_ERRORS, ids=lambda f: "+".join(x.lstrip("-") for x in f if x.startswith("--")))
def test_both_tools_refuse_exchange_without_weights_or_with_the_unweighted_flags(flags, capsys):
    """A usage error (exit status 2) with a message, before any file is read."""
    from kafka_assignment_optimizer_amd.leaders import main
    base = ["--current", "none.json", "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a"]
    with pytest.raises(SystemExit) as e:
        main(base + flags)
    err = capsys.readouterr().err
    assert e.value.code == 2 and ("--exchange needs --traffic or --sizes" in err or "cannot be combined" in err or "give one of" in err), err
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-leaders")] + base + flags, capture_output=True, cwd=ROOT)
    assert r.returncode == 2 and (b"--exchange needs --traffic or --sizes" in r.stderr or b"cannot be combined" in r.stderr or b"give one of" in r.stderr), r.stderr
    if len(flags) == 1 or "--traffic" not in flags and "--sizes" not in flags:
        assert "--exchange needs --traffic or --sizes" in err and b"--exchange needs --traffic or --sizes" in r.stderr


def test_both_tools_take_exchange_with_weights(tmp_path):
    """With --traffic the flag is accepted: the run gets past the usage checks and fails on the missing document (exit status 1)."""
    base = ["--current", str(tmp_path / "none.json"), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--traffic", str(tmp_path / "t.json"), "--exchange"]
    for prog in ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"]):
        r = subprocess.run(prog + base, capture_output=True, cwd=ROOT)
        assert r.returncode == 1, (prog, r.stderr)
        assert b"--exchange" in subprocess.run(prog + ["--help"], capture_output=True, cwd=ROOT).stdout + subprocess.run(prog + ["--help"], capture_output=True, cwd=ROOT).stderr


def test_report_line_gains_the_exchange_line_only_with_the_flag():
    from kafka_assignment_optimizer_amd.leaders import WEIGHTED_X_STAT_KEYS, WeightedLeaderResult, weighted_report_line
    kw = dict(rows=np.zeros((0, 2), dtype=np.uint16), n_changed=3, peak_before=9, peak_after=7, lower_bound=7, status="OPTIMAL_PROVEN")
    plain = weighted_report_line(WeightedLeaderResult(stats=np.arange(8), **kw))
    both = weighted_report_line(WeightedLeaderResult(stats=np.arange(12), exchange=True, exchange_rounds=8, exchanges=9, **kw))
    assert "\n" not in plain and plain.startswith("weighted: status=OPTIMAL_PROVEN ")
    assert both.splitlines() == [plain, "exchange: rounds=8 exchanges=9 proposals=10 pair_index_entries=11"]
    assert len(WEIGHTED_X_STAT_KEYS) == 12 and WEIGHTED_X_STAT_KEYS[8:] == ("exchange_rounds", "exchanges", "exchange_proposals", "pair_index_entries")


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_weighted_arrays
    with pytest.raises(kao.KaoError) as e:
        balance_leaders_weighted_arrays(np.array([[0, 1], [0, 2], [1, 2]]), 3, [4, 5, 6], exchange=True)
    assert e.value.code == -3
