"""kao_balance_logdirs_capacity and kao_place_logdirs_capacity refuse bad input on the host, before any device is
used: every refusal of their byte siblings and the three of the capacities, through the C ABI and through the Python wrappers; dir[]
stays as it is.  The readers keep totalBytes / usableBytes; the capacities file in both shapes, the precedence, the usage errors of
both command-line tools; and a run without a capacity flag writes the bytes it wrote before the flags existed."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, have_gpu

INVALID, UNSUPPORTED = -1, -2
B_ARGS = ("n_brokers", "dir_start", "base", "cap", "n_replicas", "dir", "size", "min_gain", "max_rounds", "dry_run", "n_moved", "bytes_moved", "peak_before",
          "peak_after", "per_broker", "status", "stats")
P_ARGS = ("n_brokers", "dir_start", "base", "cap", "n_replicas", "broker", "dir", "size", "move_residents", "min_gain", "max_rounds", "dry_run", "n_placed",
          "bytes_placed", "n_moved", "bytes_moved", "peak_before", "peak_after", "per_broker", "status", "stats")
GOLDEN = os.path.join(ROOT, "tests", "golden", "logdirs_cap")


def _buffers(dir_start, base, cap, dir, size, B):
    ds = np.ascontiguousarray(dir_start, dtype=np.int32)
    d = np.ascontiguousarray(dir, dtype=np.int32)
    bs = None if base is None else np.ascontiguousarray(base, dtype=np.uint64)
    cp = None if cap is None else np.ascontiguousarray(cap, dtype=np.uint64)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    return ds, d, bs, cp, sz, (len(ds) - 1 if B is None else B)


def _balance(dir_start=(0, 2, 2, 5), base=(0, 7, 0, 0, 1), cap=(10, 20, 30, 40, 50), dir=(0, 0, 1, 4, 4), size=(5, 6, 7, 8, 9), null=None, B=None, R=None, stats=False):
    """(return code, kao_last_error()) of kao_balance_logdirs_capacity; asserts that the dir buffer is unchanged after a refusal."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    ds, d, bs, cp, sz, nb = _buffers(dir_start, base, cap, dir, size, B)
    keep = d.copy()
    n, status, moved = C.c_int32(0), C.c_int32(0), C.c_uint64(0)
    peaks = np.zeros(4, dtype=np.uint64)
    per = np.zeros(10 * max(min(nb, 70000), 1), dtype=np.uint64)
    st = np.zeros(8, dtype=np.int64)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    args = [nb, ds.ctypes.data_as(i32p), None if bs is None else bs.ctypes.data_as(u64p), None if cp is None else cp.ctypes.data_as(u64p),
            d.shape[0] if R is None else R, d.ctypes.data_as(i32p), sz.ctypes.data_as(u64p), 0, 0, 0, C.byref(n), C.byref(moved), peaks[:2].ctypes.data_as(u64p),
            peaks[2:].ctypes.data_as(u64p), per.ctypes.data_as(u64p), C.byref(status), st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[B_ARGS.index(null)] = None
    rc = lib.kao_balance_logdirs_capacity(*args)
    if rc:
        assert (d == keep).all()
    return rc, lib.kao_last_error().decode()


def _place(dir_start=(0, 2, 2, 5), base=(0, 7, 0, 0, 1), cap=(10, 20, 30, 40, 50), broker=(0, 0, 0, 2, 2), dir=(0, -1, 1, 4, -1), size=(5, 6, 7, 8, 9), null=None,
           B=None, R=None, stats=False, move_residents=0):
    """(return code, kao_last_error()) of kao_place_logdirs_capacity; asserts that the dir buffer is unchanged after a refusal."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    ds, d, bs, cp, sz, nb = _buffers(dir_start, base, cap, dir, size, B)
    br = np.ascontiguousarray(broker, dtype=np.int32)
    keep = d.copy()
    n = [C.c_int32(0) for _ in range(3)]
    u = [C.c_uint64(0) for _ in range(2)]
    peaks = np.zeros(4, dtype=np.uint64)
    per = np.zeros(12 * max(min(nb, 70000), 1), dtype=np.uint64)
    st = np.zeros(10, dtype=np.int64)
    u64p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    args = [nb, ds.ctypes.data_as(i32p), None if bs is None else bs.ctypes.data_as(u64p), None if cp is None else cp.ctypes.data_as(u64p),
            d.shape[0] if R is None else R, br.ctypes.data_as(i32p), d.ctypes.data_as(i32p), sz.ctypes.data_as(u64p), move_residents, 0, 0, 0, C.byref(n[0]),
            C.byref(u[0]), C.byref(n[1]), C.byref(u[1]), peaks[:2].ctypes.data_as(u64p), peaks[2:].ctypes.data_as(u64p), per.ctypes.data_as(u64p), C.byref(n[2]),
            st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None]
    if null is not None:
        args[P_ARGS.index(null)] = None
    rc = lib.kao_place_logdirs_capacity(*args)
    if rc:
        assert (d == keep).all()
    return rc, lib.kao_last_error().decode()


CALLS = {"balance": _balance, "place": _place}
_SHARED = [
    ("null dir_start", dict(null="dir_start"), INVALID, "null pointer"),
    ("null cap", dict(null="cap"), INVALID, "null pointer"),
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
    ("dir[r] == n_dirs", dict(dir=[0, 0, 1, 5, 4]), INVALID, "dir[3]"),
    ("sizes sum to 2^62", dict(size=[2 ** 61, 2 ** 61, 0, 0, 0], base=None), INVALID, "2^62"),
    ("bases and sizes sum to 2^62", dict(base=[2 ** 61, 0, 0, 0, 2 ** 60], size=[2 ** 60, 0, 0, 0, 0]), INVALID, "2^62"),
    ("bases sum past 2^64", dict(base=[2 ** 63, 2 ** 63, 0, 0, 0]), INVALID, "2^62"),
    ("more than 4,000,000 replicas", dict(dir=[0], size=[1], R=4000001), UNSUPPORTED, "4,000,000"),
    # the capacities
    ("a capacity of 0", dict(cap=[10, 20, 0, 40, 50]), INVALID, "cap[2] is 0"),
    ("capacities sum to 2^62", dict(cap=[2 ** 61, 2 ** 61, 1, 1, 1]), INVALID, "capacities sum to 2^62"),
    ("capacities sum past 2^64", dict(cap=[2 ** 63, 2 ** 63, 2 ** 63, 1, 1]), INVALID, "capacities sum to 2^62"),
]
REFUSED = {
    "balance": _SHARED + [
        ("dir[r] below 0", dict(dir=[0, -1, 1, 4, 4]), INVALID, "dir[1]"),
        ("65 dirs on one broker", dict(dir_start=[0, 2, 67], base=None, cap=[1] * 67, dir=[0, 5], size=[1, 2]), UNSUPPORTED, "broker 1"),
    ],
    "place": [r if "replicas" not in r[0] or r[2] != UNSUPPORTED else (r[0], dict(r[1], broker=[0]), r[2], r[3]) for r in _SHARED] + [
        ("null broker", dict(null="broker"), INVALID, "null pointer"),
        ("null n_placed", dict(null="n_placed"), INVALID, "null pointer"),
        ("null bytes_placed", dict(null="bytes_placed"), INVALID, "null pointer"),
        ("broker[r] == n_brokers", dict(broker=[0, 0, 0, 3, 2]), INVALID, "broker[3]"),
        ("dir[r] below -1", dict(dir=[0, -1, -2, 4, -1]), INVALID, "dir[2]"),
        ("a resident in another broker's dir", dict(dir=[0, -1, 2, 4, -1]), INVALID, "dir[2] is not a dir of broker 0"),
        ("a homeless replica on a broker without dirs", dict(broker=[0, 1, 0, 2, 2]), INVALID, "replica 1 is homeless on broker 1"),
        ("65 dirs on one broker", dict(dir_start=[0, 2, 67], base=None, cap=[1] * 67, broker=[0, 1], dir=[0, -1], size=[1, 2]), UNSUPPORTED, "broker 1"),
    ],
}
_CASES = [(e, *r) for e in ("balance", "place") for r in REFUSED[e]]


def test_entry_points_are_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_logdirs_capacity\(int32_t n_brokers, const int32_t \*dir_start [^;]*const uint64_t \*cap /\* \[n_dirs\] \*/, int32_t n_replicas,"
                     r"[^;]*uint64_t peak_before\[2\], uint64_t peak_after\[2\],\s+uint64_t \*per_broker /\* \[n_brokers\*10\] \*/, int32_t \*status, "
                     r"int64_t stats\[8\] /\* may be NULL \*/\);", header)
    assert re.search(r"\bint kao_place_logdirs_capacity\(int32_t n_brokers, const int32_t \*dir_start [^;]*const uint64_t \*cap /\* \[n_dirs\] \*/, int32_t n_replicas, "
                     r"const int32_t \*broker[^;]*uint64_t peak_before\[2\], uint64_t peak_after\[2\],\s+uint64_t \*per_broker /\* \[n_brokers\*12\] \*/, "
                     r"int32_t \*status, int64_t stats\[10\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header   # no version bump, as for the earlier planners
    P = C.POINTER
    lib = _ffi.load()
    for name, n_args in (("kao_balance_logdirs_capacity", len(B_ARGS)), ("kao_place_logdirs_capacity", len(P_ARGS))):
        res, args = _ffi.SIGNATURES[name]
        byte_args = list(_ffi.SIGNATURES[name[:-len("_capacity")]][1])
        assert res is C.c_int and len(args) == n_args and args == byte_args[:3] + [P(C.c_uint64)] + byte_args[3:]   # the sibling's, with cap behind base
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is C.c_int


@pytest.mark.parametrize("entry,what,change,code,text", _CASES, ids=[f"{c[0]}: {c[1]}" for c in _CASES])
def test_entry_point_refuses(entry, what, change, code, text):
    for extra in (({}, dict(move_residents=1)) if entry == "place" else ({},)):
        rc, msg = CALLS[entry](**change, **extra)
        assert rc == code and msg.startswith(f"kao_{entry}_logdirs_capacity: ") and text in msg, (rc, msg)


def test_base_and_stats_may_be_null_and_limits_pass_the_host_checks():
    """None of these is a refusal: the calls get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without)."""
    want = 0 if have_gpu() else -3
    for call in (_balance, _place):
        assert call(stats=False)[0] == want and call(stats=True)[0] == want and call(base=None)[0] == want
        assert call(cap=[2 ** 61, 2 ** 60, 2 ** 59, 2 ** 58, 2 ** 58 - 1])[0] == want      # 2^62 - 1
        assert call(cap=[1, 1, 1, 1, 1])[0] == want
    assert _balance(dir_start=[0, 0, 64], base=None, cap=[3] * 64, dir=[63, 0], size=[1, 2])[0] == want
    assert _place(dir_start=[0, 0, 64], base=None, cap=[3] * 64, broker=[1, 1], dir=[63, -1], size=[1, 2], move_residents=1)[0] == want
    assert _balance(dir_start=[0, 3], base=None, cap=[1, 2, 3], dir=[0], size=[0], R=0)[0] == want


def test_the_python_wrappers_check_before_the_library():
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays, place_logdirs_arrays
    ok = dict(dir_start=[0, 2], dir=[0, 0, 1], size=[4, 5, 6])
    for bad in (dict(capacity=[1]), dict(capacity=[1, 2, 3]), dict(capacity=[1, 0]), dict(capacity=[1, -4]), dict(capacity=[1.0, 2.0]), dict(capacity=[True, 2]),
                dict(capacity=[2 ** 61, 2 ** 61]), dict(capacity=[2 ** 64, 1]), dict(capacity=[5, 6], size=[4, -5, 6]), dict(capacity=[5, 6], min_gain=2 ** 64)):
        with pytest.raises(ValueError):
            balance_logdirs_arrays(**dict(ok, **bad))
        with pytest.raises(ValueError):
            place_logdirs_arrays(**dict(ok, broker=[0, 0, 0], **bad))


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.logdirs import balance_logdirs_arrays, place_logdirs_arrays
    with pytest.raises(kao.KaoError) as e:
        balance_logdirs_arrays([0, 2], [0, 0, 1], [4, 5, 6], capacity=[10, 40])
    assert e.value.code == -3
    with pytest.raises(kao.KaoError) as e:
        place_logdirs_arrays([0, 2], [0, 0, 0], [0, -1, 1], [4, 5, 6], capacity=[10, 40])
    assert e.value.code == -3


# ---- the readers ---------------------------------------------------------------------------------------------------------------------
def _dirs_doc(total="absent", usable="absent"):
    ld = {"logDir": "/data/a", "error": None, "partitions": [{"partition": "t-0", "size": 10, "offsetLag": 0, "isFuture": False}]}
    if total != "absent":
        ld["totalBytes"] = total
    if usable != "absent":
        ld["usableBytes"] = usable
    return {"version": 1, "brokers": [{"broker": 3, "logDirs": [ld, {"logDir": "/data/b", "error": None, "partitions": []}]}]}


def test_parse_log_dirs_keeps_total_and_usable_bytes():
    from kafka_assignment_optimizer_amd.logdirs import LogDir, parse_log_dirs
    d = parse_log_dirs(_dirs_doc())[3]
    assert (d["/data/a"].total_bytes, d["/data/a"].usable_bytes) == (None, None) and d["/data/a"].entries == [("t", 0, 10, False)]
    d = parse_log_dirs(json.dumps(_dirs_doc(8000, 2 ** 53)))[3]
    assert (d["/data/a"].total_bytes, d["/data/a"].usable_bytes) == (8000, 2 ** 53) and d["/data/b"].total_bytes is None
    d = parse_log_dirs("Querying brokers\n" + json.dumps(_dirs_doc(None, 0)) + "\n")[3]
    assert (d["/data/a"].total_bytes, d["/data/a"].usable_bytes) == (None, 0)
    for bad in (dict(total=-1), dict(total=1.5), dict(total="8T"), dict(total=True), dict(usable=2 ** 53 + 1)):
        with pytest.raises(ValueError, match="Bytes"):
            parse_log_dirs(_dirs_doc(**bad))
    assert LogDir(error=None) == LogDir(error=None, entries=[], total_bytes=None, usable_bytes=None)   # two defaulted fields


def test_dir_capacities_shapes_and_precedence():
    from kafka_assignment_optimizer_amd.logdirs import dir_capacities, parse_log_dirs
    doc = {"version": 1, "brokers": [
        {"broker": 1, "logDirs": [{"logDir": "/a", "error": None, "partitions": [], "totalBytes": 1000}, {"logDir": "/b", "error": None, "partitions": [], "totalBytes": 0},
                                  {"logDir": "/c", "error": None, "partitions": []}]},
        {"broker": 2, "logDirs": [{"logDir": "/a", "error": None, "partitions": [], "totalBytes": 500}]}]}
    table = parse_log_dirs(doc)
    ids, names = [2, 1], [["/a"], ["/a", "/b", "/c"]]
    assert dir_capacities(ids, names, table, {1: {"/a": 7, "/c": "2K"}, 2: "1M", 9: 5}, 50, True) == [1 << 20, 7, 50, 2048]   # the file, then the default (totalBytes 0)
    assert dir_capacities(ids, names, table, {1: {"/b": 9}}, 50, True) == [500, 1000, 9, 50]                                   # the file, totalBytes, the default
    assert dir_capacities(ids, names, table, {1: {"/b": 9}}, 50, False) == [50, 50, 9, 50]                                    # totalBytes only when asked for
    assert dir_capacities(ids, names, table, None, 77) == [77] * 4
    assert dir_capacities(ids, names, table, {"1": 8, "2": {"/a": "3G", "/zz": 1}}) == [3 << 30, 8, 8, 8]                      # the other shape; keys as JSON has them
    with pytest.raises(ValueError, match=r"no capacity for log dirs 1:/b, 1:/c \(give"):
        dir_capacities(ids, names, table, None, None, True)
    with pytest.raises(ValueError, match="no capacity for log dirs 2:/a, 1:/a, 1:/c "):
        dir_capacities(ids, names, table, {1: {"/b": 9}})
    many = [[f"/d{i}" for i in range(8)]]
    with pytest.raises(ValueError, match="1:/d4 and 3 more"):
        dir_capacities([1], many, {1: {}}, {})
    for bad in ({1: 1.5}, {1: True}, {1: {"/a": None}}, {1: "8X"}, {1: {"/a": "abc"}}):
        with pytest.raises(ValueError, match="byte count|needs"):
            dir_capacities(ids, names, table, bad, 5)


# ---- the command-line tools: documents shared with tests/test_gpu_logdirs_cap.py -----------------------------------------------------------
EVACUATE_PAIR = (101, "/data/d1")
EVACUATE = "101:/data/d1"
PROGS = ([os.path.join(ROOT, "cli", "kao-logdirs")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.logdirs"])


def cluster_documents():
    """(current, log-dirs, capacities by dir, capacities by broker): six brokers of four dirs, /data/d0 a quarter of the others, the
    replicas placed so that the dirs hold about the same BYTES; totalBytes on every dir but two (one absent, one null), one dir with
    an error."""
    rng = np.random.default_rng(4)
    ids = [100 + i for i in range(6)]
    doc, held = {"version": 1, "partitions": []}, {b: [[] for _ in range(4)] for b in ids}
    for name, P, rf in (("alpha", 40, 3), ("be-ta", 24, 2)):
        for p in range(P):
            r = rng.permutation(6)[:rf]
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
            w = int(rng.integers(1, 1000))
            for b in r:
                held[ids[b]][int(rng.integers(0, 4))].append({"partition": f"{name}-{p}", "size": w * 1024 + int(b), "offsetLag": 0, "isFuture": False})
    held[ids[0]][1].append({"partition": "dropped-4", "size": 55555, "offsetLag": 0, "isFuture": False})   # not in --current: base
    small, large = 6 * 2 ** 20, 24 * 2 ** 20
    brokers = []
    for b in ids:
        dirs = []
        for i, e in enumerate(held[b]):
            ld = {"logDir": f"/data/d{i}", "error": None, "partitions": e, "totalBytes": small if i == 0 else large, "usableBytes": 12345}
            if (b, i) == (ids[2], 3):
                del ld["totalBytes"]
            if (b, i) == (ids[3], 2):
                ld["totalBytes"] = None
            dirs.append(ld)
        if b == ids[4]:
            dirs.append({"logDir": "/data/broken", "error": "KafkaStorageException", "partitions": [], "totalBytes": large})
        brokers.append({"broker": b, "logDirs": dirs})
    by_dir = {str(b): {f"/data/d{i}": (small if i == 0 else "24M") for i in range(4)} for b in ids}
    by_broker = {str(ids[0]): "16M", str(ids[1]): 20 * 2 ** 20}
    return doc, {"version": 1, "brokers": brokers}, by_dir, by_broker


def write_documents(tmp_path, doc, logdirs, by_dir, by_broker):
    """The documents as files, and a plan that brings four partitions to new brokers; {name: path}."""
    plan = {"version": 1, "partitions": []}
    for e in doc["partitions"][:4]:
        new = next(b for b in range(100, 106) if b not in e["replicas"])
        plan["partitions"].append({"topic": e["topic"], "partition": e["partition"], "replicas": [new] + e["replicas"][1:]})
    texts = {"current": json.dumps(doc), "logdirs": "Querying brokers for log directories information\n" + json.dumps(logdirs) + "\n",
             "caps_by_dir": json.dumps(by_dir), "caps_by_broker": json.dumps(by_broker), "plan": json.dumps(plan)}
    paths = {}
    for name, text in texts.items():
        paths[name] = str(tmp_path / f"{name}.json")
        with open(paths[name], "w") as f:
            f.write(text)
    return paths


def test_cli_usage_errors_are_equal(tmp_path):
    """Both tools: exit status 2 and the same message for a dir without a capacity, a bad --default-capacity and a bad capacities
    file; they come before any device is used."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    paths = write_documents(tmp_path, *cluster_documents())
    base = ["--current", paths["current"], "--log-dirs", paths["logdirs"], "--out", str(tmp_path / "x.json")]
    bad_files = {}
    for name, text in (("list", "[1, 2]"), ("float", '{"100": 1.5}'), ("unit", '{"100": {"/data/d0": "8X"}}'), ("id", '{"x1": 5}'), ("broken", '{"100": ')):
        bad_files[name] = str(tmp_path / f"bad_{name}.json")
        with open(bad_files[name], "w") as f:
            f.write(text)
    cases = [(["--utilisation"], "no capacity for log dirs 102:/data/d3, 103:/data/d2 (give them in --capacities, read totalBytes with --utilisation or set --default-capacity)"),
             (["--capacities", paths["caps_by_broker"]], "no capacity for log dirs 102:/data/d0, 102:/data/d1, 102:/data/d2, 102:/data/d3, 103:/data/d0 and 11 more (give"),
             (["--utilisation", "--evacuate", "102:/data/d2"], "no capacity for log dirs 102:/data/d3, 103:/data/d2 (give"),
             (["--default-capacity", "1X"], "--default-capacity needs a byte count (N, or N with K/M/G/T)"),
             (["--capacities", bad_files["list"]], "--capacities: capacities file must be a JSON object"),
             (["--capacities", bad_files["float"]], "--capacities: capacity of broker 100: not a byte count"),
             (["--capacities", bad_files["unit"]], "--capacities: capacity of log dir 100:/data/d0: not a byte count"),
             (["--capacities", bad_files["id"]], "--capacities: capacity of broker x1: not a broker id"),
             (["--capacities", bad_files["broken"]], "--capacities: "),
             (["--capacities", str(tmp_path / "none.json")], "--capacities: ")]
    for flags, text in cases:
        for prog in PROGS:
            r = subprocess.run(prog + base + flags, capture_output=True, cwd=ROOT)
            assert r.returncode == 2 and text in r.stderr.decode(), (prog, flags, r.returncode, r.stderr)
    # a capacity of 0 and capacities of 2^62 are input errors, not usage errors: exit status 1
    for flags in (["--default-capacity", "0"], ["--default-capacity", "4611686018427387904"]):
        for prog in PROGS:
            r = subprocess.run(prog + base + flags, capture_output=True, cwd=ROOT)
            assert r.returncode == 1 and b"kao-logdirs: " in r.stderr, (prog, flags, r.stderr)


def test_a_run_without_capacity_flags_writes_what_it_wrote_before(tmp_path):
    """The plan and the report of both tools, without a capacity flag, on documents that carry totalBytes and on examples/current.json:
    byte for byte the files that the tools wrote before the flags existed (tests/golden/logdirs_cap; the launch count aside, they hold
    no number that depends on the device).  Without a device both fail as they did: exit status 1 and the library's message."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    doc, logdirs, by_dir, by_broker = cluster_documents()
    paths = write_documents(tmp_path, doc, logdirs, by_dir, by_broker)
    example = json.load(open(os.path.join(ROOT, "examples", "current.json")))
    ex_dirs = {"version": 1, "brokers": [{"broker": b, "logDirs": [
        {"logDir": f"/data/{n}", "error": None, "totalBytes": 2 ** 30 if n == "a" else 2 ** 32,
         "partitions": [{"partition": f"{e['topic']}-{e['partition']}", "size": 1000 * (j + 1) + e["partition"], "offsetLag": 0, "isFuture": False}
                        for e in example["partitions"] for j, x in enumerate(e["replicas"]) if x == b and (n == "a") == (e["partition"] % 3 != 0)]}
        for n in ("a", "b")]} for b in range(20)]}
    with open(tmp_path / "ex_dirs.json", "w") as f:
        json.dump(ex_dirs, f)
    runs = {"cluster": ["--current", paths["current"], "--log-dirs", paths["logdirs"]],
            "cluster_place": ["--current", paths["current"], "--log-dirs", paths["logdirs"], "--plan", paths["plan"], "--evacuate", EVACUATE, "--rebalance"],
            "example": ["--current", os.path.join(ROOT, "examples", "current.json"), "--log-dirs", str(tmp_path / "ex_dirs.json")]}
    for tag, args in runs.items():
        for i, prog in enumerate(PROGS):
            out = tmp_path / f"{tag}{i}.json"
            r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
            if not have_gpu():
                assert r.returncode == 1 and b"kao-logdirs: " in r.stderr and not out.exists()
                continue
            assert r.returncode == 0, r.stderr
            assert out.read_bytes() == open(os.path.join(GOLDEN, f"{tag}_plan.json"), "rb").read()
            assert r.stderr.decode() == open(os.path.join(GOLDEN, f"{tag}_report.txt")).read()
