"""kao_balance_disk_exchange refuses bad input on the host, before any device is used: the shared refusals of
tests/test_disk_errors.py against the new symbol, each with its return code and the new prefix in kao_last_error(), the text behind
the prefix the plain call's; the rows stay as they are.  The limit of the member index is checked on the host.  The entry point is
declared, exported and bound, both command-line tools refuse --exchange with the budget and capacity flags, and without a device a
valid call fails loudly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_disk_errors as shared
from conftest import ROOT, have_gpu

PREFIX = "kao_balance_disk_exchange: "


def _call(rows=((0, 1), (2, 3), (1, 2)), B=4, R=2, rack_of=None, size=(5, 6, 7), null=None, P=None, W=None, stats=True):
    """(return code, kao_last_error()); asserts that the row buffer and the stats are unchanged on error."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    rk = np.ascontiguousarray(np.arange(max(B, 1)) % max(R, 1) if rack_of is None else rack_of, dtype=np.uint8)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    n, status = C.c_int32(0), C.c_int32(0)
    u = [C.c_uint64(0) for _ in range(4)]
    st = np.full(12, -7, dtype=np.int64)
    args = [B, R, rk.ctypes.data_as(C.POINTER(C.c_uint8)), r.shape[0] if P is None else P, r.shape[1] if W is None else W,
            r.ctypes.data_as(C.POINTER(C.c_uint16)), sz.ctypes.data_as(C.POINTER(C.c_uint64)), 0, 1, 0, 0, 0, C.byref(n), C.byref(u[0]), C.byref(u[1]),
            C.byref(u[2]), C.byref(u[3]), C.byref(status), st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[shared.ARGS.index(null)] = None
    rc = lib.kao_balance_disk_exchange(*args)
    if rc:
        assert (r == keep).all() and (st == -7).all()   # a rejected call leaves the rows and the stats alone
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_disk_exchange\(int32_t n_brokers, int32_t n_racks, const uint8_t \*rack_of, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/, const uint64_t \*size /\* \[n_partitions\] \*/,\s+"
                     r"int32_t max_per_rack /\* <= 0: no rack rule \*/, int32_t move_leaders, uint64_t min_gain,\s+"
                     r"int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run, int32_t \*n_moved, uint64_t \*bytes_moved,\s+"
                     r"uint64_t \*peak_before, uint64_t \*peak_after, uint64_t \*lower_bound, int32_t \*status,\s+"
                     r"int64_t stats\[12\] /\* may be NULL \*/\);", header)
    assert "#define KAO_DISK_EXCHANGE_MAX_WORDS (1ull << 27)" in header and "#define KAO_VERSION 103" in header   # no version bump
    res, args = _ffi.SIGNATURES["kao_balance_disk_exchange"]
    assert res is C.c_int and args == _ffi.SIGNATURES["kao_balance_disk"][1] and len(args) == len(shared.ARGS)
    bound = _ffi.load().kao_balance_disk_exchange
    assert bound.argtypes == args and bound.restype is C.c_int


@pytest.mark.parametrize("what,change,code,text", shared.REFUSED, ids=[r[0] for r in shared.REFUSED])
def test_entry_point_refuses(what, change, code, text):
    """The plain call's refusal with the new prefix, the same return code and the same text behind the prefix."""
    from kafka_assignment_optimizer_amd import _ffi
    rc, msg = _call(**change)
    assert rc == code and msg.startswith(PREFIX) and text in msg, (rc, msg)
    assert shared._call(**change) == (code, "kao_balance_disk: " + msg[len(PREFIX):])


def test_index_limit_is_checked_on_the_host():
    """8,000 brokers and N = 1,100,000 positive sizes: 8000 * ceil(N / 64) = 137,504,000 mask words, above 2^27 = 134,217,728.  With every
    second size zero (68,752,000 words) the same rows pass the host checks; that is tried only where no device would then run them."""
    P = 1100000
    rows = np.zeros((P, 1), dtype=np.uint16)
    rc, msg = _call(rows=rows, B=8000, R=1, size=np.ones(P, dtype=np.uint64))
    assert rc == -2 and msg.startswith(PREFIX) and "2^27" in msg, (rc, msg)
    if not have_gpu():
        assert _call(rows=rows, B=8000, R=1, size=np.arange(P, dtype=np.uint64) % 2)[0] == -3
        assert shared._call(rows=rows, B=8000, R=1, size=np.ones(P, dtype=np.uint64))[0] == -3   # the plain call has no such limit


def test_stats_may_be_null_and_sizes_just_below_the_limit_pass_the_host_checks():
    """Neither is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    assert _call(stats=False)[0] == want and _call(stats=True)[0] == want
    assert _call(size=[2 ** 60 - 1, 2 ** 60, 0])[0] == want
    assert _call(rows=np.zeros((0, 2)), size=np.zeros(1), P=0)[0] == want   # no partition


FLAG_ERRORS = [["--max-bytes", "1G"], ["--capacities", "0:1G,1:1G,2:1G"], ["--default-capacity", "1G"], ["--max-bytes", "5", "--default-capacity", "1G"]]


@pytest.mark.parametrize("flags", FLAG_ERRORS, ids=lambda f: "+".join(x.lstrip("-") for x in f if x.startswith("--")))
def test_both_tools_refuse_exchange_with_the_budget_and_capacity_flags(flags, capsys):
    """A usage error (exit status 2) with a message, before any file is read; the flags alone get past the usage checks."""
    from kafka_assignment_optimizer_amd.disk import main
    base = ["--current", "none.json", "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--sizes", "none.txt", "--out", "none.out"]
    with pytest.raises(SystemExit) as e:
        main(base + ["--exchange"] + flags)
    assert e.value.code == 2 and "--exchange works by bytes only" in capsys.readouterr().err
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    tool = os.path.join(ROOT, "cli", "kao-disk")
    r = subprocess.run([tool] + base + flags + ["--exchange"], capture_output=True, cwd=ROOT)
    assert r.returncode == 2 and b"--exchange works by bytes only" in r.stderr, r.stderr
    assert subprocess.run([tool] + base + flags, capture_output=True, cwd=ROOT).returncode == 1   # the missing document, not the usage
    assert main(base + flags) == 1


def test_both_tools_take_exchange_alone_and_name_it_in_their_help(tmp_path):
    base = ["--current", str(tmp_path / "none.json"), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--sizes", str(tmp_path / "s.txt"), "--out",
            str(tmp_path / "o.json"), "--exchange", "--max-per-rack", "1", "--keep-leaders", "--min-gain", "1K", "--max-rounds", "3", "--dry-run", "--report"]
    for prog in ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"]):
        r = subprocess.run(prog + base, capture_output=True, cwd=ROOT)
        assert r.returncode == 1, (prog, r.stderr)   # past the usage checks: the missing document
        h = subprocess.run(prog + ["--help"], capture_output=True, cwd=ROOT)
        assert b"--exchange" in h.stdout + h.stderr


def test_python_api_refuses_exchange_with_a_budget_or_capacities():
    from kafka_assignment_optimizer_amd.disk import EXCHANGE_STAT_KEYS, DiskResult, balance_disk, balance_disk_arrays
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    for kw in (dict(max_bytes=10), dict(capacity=[5, 5, 5]), dict(max_bytes=0, capacity=[5, 5, 5])):
        with pytest.raises(ValueError, match="by bytes only"):
            balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], exchange=True, **kw)
    with pytest.raises(ValueError, match="by bytes only"):
        balance_disk({"version": 1, "partitions": []}, {}, broker_list=[0, 1], racks={0: "a", 1: "a"}, exchange=True, max_bytes=1)
    assert len(EXCHANGE_STAT_KEYS) == 12 and EXCHANGE_STAT_KEYS[8:] == ("exchange_rounds", "exchanges", "exchange_proposals", "peak_of_moves")
    assert {"exchange_rounds", "exchanges", "exchange_proposals", "peak_of_moves"} <= set(DiskResult.__dataclass_fields__)


def test_report_line_gains_the_exchange_numbers_only_with_the_flag():
    from kafka_assignment_optimizer_amd.disk import DiskPlan, DiskResult, report_lines
    from kafka_assignment_optimizer_amd.failover import parse_current
    fi = parse_current({"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [0, 1]}]}, [0, 1], {0: "a", 1: "a"})
    kw = dict(rows=fi.rows, n_moved=3, bytes_moved=30, peak_before=9, peak_after=7, lower_bound=7, status="OPTIMAL_PROVEN")
    plain = report_lines(DiskPlan(DiskResult(stats=np.array([0, 1, 2, 3, 4, 5, 1, 7]), **kw), fi, np.array([5], dtype=np.uint64)))
    both = report_lines(DiskPlan(DiskResult(stats=np.array([0, 1, 2, 3, 4, 5, 1, 7, 8, 9, 10, 11]), exchange_rounds=8, exchanges=9, exchange_proposals=10, peak_of_moves=11, **kw), fi,
                                 np.array([5], dtype=np.uint64)))
    assert len(plain) == len(both) == 1 and both[0] == plain[0] + " peak_of_moves=11 exchange_rounds=8 exchanges=9 exchange_proposals=10"


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.disk import balance_disk_arrays
    with pytest.raises(kao.KaoError) as e:
        balance_disk_arrays(np.array([[0, 1], [0, 2], [1, 2]]), 3, [0, 0, 0], 1, [4, 5, 6], exchange=True)
    assert e.value.code == -3 and "kao_balance_disk_exchange" in str(e.value)
