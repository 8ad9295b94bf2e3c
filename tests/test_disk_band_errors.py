"""kao_balance_disk_banded refuses bad input on the host, before any device is used: the shared refusals of
tests/test_disk_errors.py against the new symbol with the new prefix, with and without exchange, a band that is no band and a null
count_range; the rows, the stats and the outputs stay as they are.  The entry point is declared, exported and bound; both command-line
tools refuse --replica-band and --count-slack together, with the budget, capacity and drain flags, and a band that does not parse; the
Python API refuses the same before the library is loaded; --count-slack is floor(R / B) - K : ceil(R / B) + K with LO clipped at 0; the
report line of the Python twin is the C++ tool's; without a device a valid call fails loudly."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_disk_errors as shared
from conftest import ROOT, have_gpu

PREFIX = "kao_balance_disk_banded: "
ARGS = shared.ARGS[:7] + ("count_lo", "count_hi", "exchange") + shared.ARGS[7:17] + ("count_range",) + shared.ARGS[17:]


def _call(rows=((0, 1), (2, 3), (1, 2)), B=4, R=2, rack_of=None, size=(5, 6, 7), null=None, P=None, W=None, stats=True, lo=0, hi=3, exchange=0):
    """(return code, kao_last_error()); asserts that the row buffer, the stats and the outputs are unchanged on error."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    rk = np.ascontiguousarray(np.arange(max(B, 1)) % max(R, 1) if rack_of is None else rack_of, dtype=np.uint8)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    n, status = C.c_int32(-7), C.c_int32(-7)
    u = [C.c_uint64(77) for _ in range(4)]
    counts = (C.c_int32 * 4)(-7, -7, -7, -7)
    st = np.full(14, -7, dtype=np.int64)
    args = [B, R, rk.ctypes.data_as(C.POINTER(C.c_uint8)), r.shape[0] if P is None else P, r.shape[1] if W is None else W,
            r.ctypes.data_as(C.POINTER(C.c_uint16)), sz.ctypes.data_as(C.POINTER(C.c_uint64)), lo, hi, exchange, 0, 1, 0, 0, 0, C.byref(n),
            C.byref(u[0]), C.byref(u[1]), C.byref(u[2]), C.byref(u[3]), counts, C.byref(status), st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[ARGS.index(null)] = None
    rc = lib.kao_balance_disk_banded(*args)
    if rc:   # a rejected call leaves the rows, the stats and every output alone
        assert (r == keep).all() and (st == -7).all() and (n.value, status.value) == (-7, -7) and all(x.value == 77 for x in u) and list(counts) == [-7] * 4
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_disk_banded\(int32_t n_brokers, int32_t n_racks, const uint8_t \*rack_of, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/, const uint64_t \*size /\* \[n_partitions\] \*/,\s+"
                     r"int32_t count_lo, int32_t count_hi, int32_t exchange /\* != 0: exchange rounds as well \*/,\s+"
                     r"int32_t max_per_rack /\* <= 0: no rack rule \*/, int32_t move_leaders, uint64_t min_gain,\s+"
                     r"int32_t max_rounds /\* <= 0: no limit \*/, int32_t dry_run, int32_t \*n_moved, uint64_t \*bytes_moved,\s+"
                     r"uint64_t \*peak_before, uint64_t \*peak_after, uint64_t \*lower_bound, int32_t count_range\[4\],\s+"
                     r"int32_t \*status, int64_t stats\[14\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header   # no version bump, as for the earlier planners
    res, args = _ffi.SIGNATURES["kao_balance_disk_banded"]
    plain = _ffi.SIGNATURES["kao_balance_disk"][1]
    P = C.POINTER
    assert res is C.c_int and len(args) == len(ARGS) and args == plain[:7] + [C.c_int32] * 3 + plain[7:17] + [P(C.c_int32)] + plain[17:]
    bound = _ffi.load().kao_balance_disk_banded
    assert bound.argtypes == args and bound.restype is C.c_int


@pytest.mark.parametrize("exchange", [0, 1])
@pytest.mark.parametrize("what,change,code,text", shared.REFUSED, ids=[r[0] for r in shared.REFUSED])
def test_entry_point_refuses_what_the_plain_call_refuses(what, change, code, text, exchange):
    """The plain call's refusal with the new prefix, the same return code and the same text behind the prefix."""
    rc, msg = _call(exchange=exchange, **change)
    assert rc == code and msg.startswith(PREFIX) and text in msg, (rc, msg)
    assert shared._call(**change) == (code, "kao_balance_disk: " + msg[len(PREFIX):])


NEW_REFUSED = [
    ("null count_range", dict(null="count_range"), "null pointer"),
    ("count_lo below 0", dict(lo=-1, hi=3), "count_lo < 0"),
    ("count_hi below count_lo", dict(lo=2, hi=1), "count_hi < count_lo"),
    ("both below 0", dict(lo=-2, hi=-1), "count_lo < 0"),
]


@pytest.mark.parametrize("exchange", [0, 1])
@pytest.mark.parametrize("what,change,text", NEW_REFUSED, ids=[r[0] for r in NEW_REFUSED])
def test_entry_point_refuses_the_new_cases(what, change, text, exchange):
    rc, msg = _call(exchange=exchange, **change)
    assert rc == shared.INVALID and msg.startswith(PREFIX) and text in msg, (rc, msg)


def test_the_mask_word_limit_of_the_exchange_call_holds_with_exchange_only():
    """8,000 brokers x 2^20 partitions of size > 0 are 2^27 + mask words: refused with exchange, as kao_balance_disk_exchange refuses it
    (the rows are valid: a refusal of the shared checks would come first)."""
    P, B = 1 << 21, 8000
    rows = (np.arange(P, dtype=np.uint16) % B).reshape(P, 1)
    size = np.ones(P, dtype=np.uint64)
    rc, msg = _call(rows=rows, B=B, R=1, size=size, exchange=1, hi=P)
    assert rc == shared.UNSUPPORTED and msg.startswith(PREFIX) and "2^27 mask words" in msg, (rc, msg)


def test_the_shared_checks_come_before_the_band():
    rc, msg = _call(rows=[[0, 1], [3, 3], [1, 2]], lo=5, hi=2)
    assert rc == shared.INVALID and "partition 1" in msg


def test_valid_calls_pass_the_host_checks():
    """None is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without).  A band the total replica
    count cannot satisfy is no error: nothing is forced."""
    want = 0 if have_gpu() else -3
    assert _call(stats=False)[0] == want and _call(stats=True)[0] == want and _call(exchange=1)[0] == want
    assert _call(lo=0, hi=0)[0] == want and _call(lo=100, hi=100)[0] == want and _call(lo=0, hi=2 ** 31 - 1, exchange=7)[0] == want
    assert _call(rows=np.zeros((0, 2)), size=np.zeros(1), P=0)[0] == want              # no partition


BASE = ["--current", "none.json", "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--sizes", "none.txt", "--out", "none.out"]
BY_BYTES = " works by bytes only: not together with --max-bytes, --capacities, --default-capacity or --drain"
FLAG_ERRORS = [(["--replica-band", "1:2", "--count-slack", "1"], "--replica-band and --count-slack: give one of the two"),
               (["--replica-band", "1:2", "--max-bytes", "1G"], "--replica-band" + BY_BYTES), (["--replica-band", "1:2", "--capacities", "0:1G,1:1G,2:1G"], "--replica-band" + BY_BYTES),
               (["--replica-band", "1:2", "--default-capacity", "1G"], "--replica-band" + BY_BYTES), (["--replica-band", "1:2", "--drain", "1"], "--replica-band" + BY_BYTES),
               (["--count-slack", "1", "--max-bytes", "1G"], "--count-slack" + BY_BYTES), (["--count-slack", "1", "--capacities", "0:1G,1:1G,2:1G"], "--count-slack" + BY_BYTES),
               (["--count-slack", "1", "--default-capacity", "1G"], "--count-slack" + BY_BYTES), (["--count-slack", "1", "--drain", "1", "--exchange"], "--drain works by bytes only"),
               (["--count-slack", "1", "--drain", "1"], "--count-slack" + BY_BYTES),
               (["--replica-band", "3:2"], "--replica-band: HI is below LO"), (["--replica-band", "3"], "--replica-band needs LO:HI"),
               (["--replica-band", "a:3"], "--replica-band needs LO:HI"), (["--replica-band", "1:x"], "--replica-band needs LO:HI"),
               (["--replica-band", "1:"], "--replica-band needs LO:HI"), (["--count-slack", "x"], "--count-slack needs a count"),
               (["--count-slack", "-1"], "--count-slack needs a count")]


@pytest.mark.parametrize("flags,text", FLAG_ERRORS, ids=["+".join(f[0]) for f in FLAG_ERRORS])
def test_both_tools_refuse(flags, text, capsys):
    """A usage error (exit status 2) with a message that names the flag, before any file is read."""
    from kafka_assignment_optimizer_amd.disk import main
    with pytest.raises(SystemExit) as e:
        main(BASE + flags)
    assert e.value.code == 2 and text in capsys.readouterr().err
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-disk")] + BASE + flags, capture_output=True, cwd=ROOT)
    assert r.returncode == 2 and text.encode() in r.stderr, r.stderr


@pytest.mark.parametrize("band", [["--replica-band", "0:5"], ["--count-slack", "2"]], ids=["band", "slack"])
@pytest.mark.parametrize("exchange", [[], ["--exchange"]], ids=["moves", "exchange"])
def test_both_tools_take_the_flags_with_every_other_option_and_document_them(tmp_path, band, exchange):
    base = ["--current", str(tmp_path / "none.json"), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--sizes", str(tmp_path / "s.txt"), "--out",
            str(tmp_path / "o.json"), "--max-per-rack", "1", "--keep-leaders", "--min-gain", "1K", "--max-rounds", "3", "--dry-run", "--report"] + band + exchange
    for prog in ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"]):
        r = subprocess.run(prog + base, capture_output=True, cwd=ROOT)
        assert r.returncode == 1, (prog, r.stderr)   # past the usage checks: the missing document
        h = subprocess.run(prog + ["--help"], capture_output=True, cwd=ROOT)
        assert b"--replica-band" in h.stdout + h.stderr and b"--count-slack" in h.stdout + h.stderr


def test_both_tools_report_the_same_on_an_error_and_on_a_usage_error(tmp_path):
    """A refused case (the document names a broker outside the list: exit status 1) and a usage error without --dry-run (exit status 2):
    the Python twin's stderr ends as the C++ tool's does, and neither writes the plan."""
    cur = tmp_path / "cur.json"
    cur.write_text('{"version":1,"partitions":[{"topic":"t","partition":0,"replicas":[0,9]}]}')
    sizes = tmp_path / "s.json"
    sizes.write_text('{"partitions":[{"topic":"t","partition":0,"size":5}]}')
    base = ["--current", str(cur), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a", "--sizes", str(sizes), "--report"]
    last = []
    for flags, status in ((["--count-slack", "1", "--exchange"], 1), (["--replica-band", "2:1"], 2)):
        for i, prog in enumerate(([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"])):
            out = tmp_path / f"o{i}.json"
            r = subprocess.run(prog + base + flags + ["--out", str(out)], capture_output=True, cwd=ROOT)
            assert r.returncode == status and not out.exists(), (prog, r.stderr)
            last.append([l for l in r.stderr.decode().splitlines() if l.startswith("kao-disk: ")][-1])
    assert last[0] == last[1] and "9" in last[0]
    assert last[2].startswith("kao-disk: --replica-band: HI is below LO") and last[3].startswith("kao-disk: ") and "--replica-band: HI is below LO" in last[3]


def test_count_slack_arithmetic():
    from kafka_assignment_optimizer_amd.disk import slack_band
    assert slack_band(10, 3, 0) == (3, 4) and slack_band(10, 3, 1) == (2, 5) and slack_band(9, 3, 0) == (3, 3) and slack_band(9, 3, 2) == (1, 5)
    assert slack_band(2, 5, 0) == (0, 1) and slack_band(2, 5, 3) == (0, 4) and slack_band(10, 3, 7) == (0, 11)   # LO clipped at 0
    assert slack_band(0, 4, 0) == (0, 0) and slack_band(3600, 12, 1) == (299, 301)
    for bad in (-1, 1.5, True, "1"):
        with pytest.raises(ValueError, match="count_slack"):
            slack_band(10, 3, bad)


def test_python_api_refuses_before_the_library_is_loaded():
    from kafka_assignment_optimizer_amd.disk import BANDED_STAT_KEYS, DiskResult, balance_disk, balance_disk_arrays
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    for kw in (dict(max_bytes=10), dict(capacity=[5, 5, 5]), dict(drain=[1, 0, 0]), dict(max_bytes=0, capacity=[5, 5, 5])):
        with pytest.raises(ValueError, match="count_band works by bytes only"):
            balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], count_band=(1, 2), **kw)
    for band, text in (((-1, 2), "lo must be >= 0"), ((2, 1), "hi must be >= lo"), ((1.0, 2), "must be integers"), ((True, 2), "must be integers"), (3, "pair"),
                       ((1, 2, 3), "pair")):
        for exchange in (False, True):
            with pytest.raises(ValueError, match=text):
                balance_disk_arrays(rows, 3, [0, 0, 0], 1, [4, 5, 6], count_band=band, exchange=exchange)
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [0, 1]}]}
    kw = dict(broker_list=[0, 1], racks={0: "a", 1: "a"})
    with pytest.raises(ValueError, match="give one of the two"):
        balance_disk(doc, {("t", 0): 5}, count_band=(0, 1), count_slack=1, **kw)
    for more in (dict(max_bytes=1), dict(capacity={0: 5, 1: 5}), dict(drain=[1])):
        for band in (dict(count_band=(0, 1)), dict(count_slack=1)):
            with pytest.raises(ValueError, match="count_band works by bytes only"):
                balance_disk(doc, {("t", 0): 5}, **band, **more, **kw)
    with pytest.raises(ValueError, match="count_slack"):
        balance_disk(doc, {("t", 0): 5}, count_slack=-1, **kw)
    with pytest.raises(ValueError, match="hi must be >= lo"):
        balance_disk(doc, {("t", 0): 5}, count_band=(3, 2), **kw)
    assert len(BANDED_STAT_KEYS) == 14 and BANDED_STAT_KEYS[8:] == ("exchange_rounds", "exchanges", "exchange_proposals", "peak_of_moves", "outside_band", "outside_band_before")
    assert {"count_band", "count_range", "outside_band", "outside_band_before"} <= set(DiskResult.__dataclass_fields__)


def test_report_gains_one_line_for_the_band():
    from kafka_assignment_optimizer_amd.disk import DiskPlan, DiskResult, report_lines
    from kafka_assignment_optimizer_amd.failover import parse_current
    doc = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [10, 11]}, {"topic": "t", "partition": 1, "replicas": [10]}]}
    fi = parse_current(doc, [10, 11, 12], {10: "a", 11: "b", 12: "b"})
    kw = dict(rows=fi.rows, n_moved=3, bytes_moved=30, peak_before=9, peak_after=7, lower_bound=7, status="FEASIBLE_BOUND_GAP")
    size = np.array([5, 2], dtype=np.uint64)
    plain = report_lines(DiskPlan(DiskResult(stats=np.array([0, 1, 2, 3, 4, 5, 1, 7]), **kw), fi, size))
    band = dict(count_band=(1, 1), count_range=(0, 2, 1, 1), outside_band=0, outside_band_before=2)
    stats = np.array([0, 1, 2, 3, 4, 5, 1, 7, 8, 9, 10, 11, 0, 2])
    line = "disk: replica_band=1:1 counts_before=0..2 counts_after=1..1 outside_before=2 outside_after=0"
    assert len(plain) == 1 and report_lines(DiskPlan(DiskResult(stats=stats, **band, **kw), fi, size)) == [plain[0], line]
    x = dict(exchange_rounds=8, exchanges=9, exchange_proposals=10, peak_of_moves=11)
    assert report_lines(DiskPlan(DiskResult(stats=stats, **band, **x, **kw), fi, size)) == [
        plain[0] + " peak_of_moves=11 exchange_rounds=8 exchanges=9 exchange_proposals=10", line]


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.disk import balance_disk_arrays
    for exchange in (False, True):
        with pytest.raises(kao.KaoError) as e:
            balance_disk_arrays(np.array([[0, 1], [0, 2], [1, 2]]), 3, [0, 0, 0], 1, [4, 5, 6], count_band=(1, 3), exchange=exchange)
        assert e.value.code == -3 and "kao_balance_disk_banded" in str(e.value)
