"""kao_plan_waves_headroom refuses bad input on the host, before any device is used, with kao_last_error()
naming the argument; the entry point is declared, exported and bound; the Python layer derives stored bytes and capacities from
its sources in the documented order and names what is missing; both command-line tools refuse the new flags' misuse."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, have_gpu

NONE = 0xFFFF
PREFIX = "kao_plan_waves_headroom: "
CUR = ((0, 1), (2, 3))
TGT = ((0, 4), (2, 3))


def _call(B=5, cur=CUR, tgt=TGT, size=(10, 20), stored=(10, 10, 20, 20, 0), capacity=(100,) * 5, cap=0, k=0, null=None, W=None, stats=True):
    """(return code, kao_last_error()); a refused call leaves the outputs alone."""
    from kafka_assignment_optimizer_amd import _ffi
    lib = _ffi.load()
    c = np.ascontiguousarray(cur, dtype=np.uint16)
    t = np.ascontiguousarray(tgt, dtype=np.uint16)
    sz, sto, cp = (np.ascontiguousarray(v, dtype=np.uint64) for v in (size, stored, capacity))
    P = c.shape[0]
    wave = np.full(max(P, 1), -7, dtype=np.int32)
    st = np.full(8, -7, dtype=np.int64)
    nw, lb = C.c_int32(-7), C.c_int32(-7)
    u16, u64, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    args = dict(current=c.ctypes.data_as(u16), target=t.ctypes.data_as(u16), size=sz.ctypes.data_as(u64), stored=sto.ctypes.data_as(u64),
                capacity=cp.ctypes.data_as(u64), wave=wave.ctypes.data_as(i32), n_waves=C.byref(nw), lower_bound=C.byref(lb))
    if null is not None:
        args[null] = None
    rc = lib.kao_plan_waves_headroom(B, P, c.shape[1] if W is None else W, args["current"], args["target"], args["size"], args["stored"],
                                     args["capacity"], cap, k, 1, args["wave"], args["n_waves"], args["lower_bound"],
                                     st.ctypes.data_as(C.POINTER(C.c_int64)) if stats else None)
    if rc == -1:
        assert (wave == -7).all() and (st == -7).all() and nw.value == lb.value == -7
    return rc, lib.kao_last_error().decode()


def test_entry_point_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_plan_waves_headroom\(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t \*current, "
                     r"const uint16_t \*target,\s+const uint64_t \*size /\* \[n_partitions\] bytes \*/, const uint64_t \*stored /\* \[n_brokers\] bytes \*/,\s+"
                     r"const uint64_t \*capacity /\* \[n_brokers\] bytes \*/, uint64_t max_bytes_per_broker, int32_t max_per_broker,\s+"
                     r"uint64_t seed, int32_t \*wave /\* \[n_partitions\] \*/, int32_t \*n_waves, int32_t \*lower_bound,\s+"
                     r"int64_t stats\[8\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header   # no version bump
    res, args = _ffi.SIGNATURES["kao_plan_waves_headroom"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [C.c_int32, C.c_int32, C.c_int32, P(C.c_uint16), P(C.c_uint16), P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), C.c_uint64,
                    C.c_int32, C.c_uint64, P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_int64)]
    fn = _ffi.load().kao_plan_waves_headroom
    assert fn.argtypes == args and fn.restype is C.c_int


REFUSED = [
    ("null current", dict(null="current"), "null pointer"),
    ("null target", dict(null="target"), "null pointer"),
    ("null wave", dict(null="wave"), "null pointer"),
    ("null n_waves", dict(null="n_waves"), "null pointer"),
    ("null lower_bound", dict(null="lower_bound"), "null pointer"),
    ("null size", dict(null="size"), "null size"),
    ("null stored", dict(null="stored"), "null stored"),
    ("null capacity", dict(null="capacity"), "null capacity"),
    ("width 0", dict(W=0), "width must be 1..8"),
    ("width 9", dict(W=9), "width must be 1..8"),
    ("no broker", dict(B=0), "n_brokers must be 1..65534"),
    ("too many brokers", dict(B=65535), "n_brokers must be 1..65534"),
    ("broker index", dict(B=4, stored=(10, 10, 20, 20), capacity=(100,) * 4), "broker index 4 >= n_brokers"),
    ("broker repeated", dict(tgt=((0, 0), (2, 3))), "broker repeated in a row"),
    ("empty target row", dict(tgt=((NONE, NONE), (2, 3))), "target row has no broker"),
    ("negative count cap", dict(k=-1), "max_per_broker must be >= 0"),
    # broker 4 receives 2^62 bytes in all (two partitions of 2^61)
    ("traffic 2^62", dict(cur=((0, 1), (2, 3)), tgt=((4, 1), (4, 3)), size=(1 << 61, 1 << 61), stored=((1 << 61),) * 4 + (0,)),
     "a broker's traffic reaches 2^62 bytes"),
    ("n_added x size overflows", dict(B=8, cur=((0, 1, 2),), tgt=((5, 6, 7),), size=((1 << 64) - 1,), stored=(0,) * 8, capacity=(0,) * 8),
     "a broker's traffic reaches 2^62 bytes"),
    ("stored 2^62", dict(stored=(10, 10, 20, 1 << 62, 0)), "stored[3] reaches 2^62 bytes"),
    # partition 0 leaves broker 1 with 10 bytes, of which broker 1 stores 9
    ("stored below what leaves", dict(stored=(10, 9, 20, 20, 0)), "stored[1] is below the bytes of the partitions that leave the broker"),
    # a metadata-only partition leaves too: partition 1 drops broker 3
    ("stored below a metadata-only removal", dict(tgt=((0, 1), (2, NONE)), stored=(10, 10, 20, 19, 0)),
     "stored[3] is below the bytes of the partitions that leave the broker"),
    # two partitions leave broker 1: 10 + 20 bytes against 29 stored
    ("stored below the sum of what leaves", dict(cur=((0, 1), (2, 1)), tgt=((0, 4), (2, 3)), stored=(10, 29, 20, 0, 0)),
     "stored[1] is below the bytes of the partitions that leave the broker"),
]


@pytest.mark.parametrize("what,change,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_entry_point_refuses(what, change, text):
    rc, msg = _call(**change)
    assert rc == -1 and msg.startswith(PREFIX) and text in msg, (rc, msg)


def test_what_is_not_a_refusal():
    """These get as far as the device (KAO_OK with one, KAO_ERR_NO_DEVICE without): no cap at all, stats == NULL, stored exactly what
    leaves, stored just below 2^62, capacities of any size, sizes of partitions that move nothing."""
    want = 0 if have_gpu() else -3
    assert _call()[0] == want                                   # k = C = 0
    assert _call(stats=False)[0] == want
    assert _call(cap=5, k=2)[0] == want
    assert _call(stored=(0, 10, 0, 0, 0))[0] == want            # broker 1 stores exactly the 10 bytes that leave it
    assert _call(stored=((1 << 62) - 1,) * 5, capacity=((1 << 64) - 1, 0, 1 << 63, 5, 5))[0] == want
    assert _call(tgt=CUR, size=((1 << 64) - 1,) * 2, stored=(0,) * 5)[0] == want
    assert _call(cur=np.zeros((0, 2)), tgt=np.zeros((0, 2)), size=np.zeros(1))[0] == want


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.waves import plan_waves, plan_waves_headroom_arrays
    with pytest.raises(kao.KaoError) as e:
        plan_waves_headroom_arrays(np.array(CUR), np.array(TGT), 5, [10, 20], [10, 10, 20, 20, 0], [100] * 5)
    assert e.value.code == -3 and "kao_plan_waves_headroom" in str(e.value)
    with pytest.raises(kao.KaoError):
        plan_waves(*_documents()[:2], sizes=_documents()[2], default_capacity=1 << 30)


def _documents():
    """current, plan and a kafka-log-dirs document: brokers 1 and 2 report totalBytes for every dir, broker 3 for one dir of two,
    broker 4 is not in the document; broker 1 also holds a future replica and a partition outside the assignment."""
    cur = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [1, 2]}, {"topic": "t", "partition": 1, "replicas": [2, 3]},
                                        {"topic": "t", "partition": 2, "replicas": [3, 1]}]}
    plan = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [4, 2]}, {"topic": "t", "partition": 1, "replicas": [2, 1]}]}

    def entry(p, size, future=False):
        return {"partition": f"t-{p}", "size": size, "offsetLag": 0, "isFuture": future}
    logdirs = {"version": 1, "brokers": [
        {"broker": 1, "logDirs": [{"logDir": "/a", "error": None, "totalBytes": 600, "usableBytes": 1, "partitions": [entry(0, 100), entry(2, 290)]},
                                  {"logDir": "/b", "error": None, "totalBytes": 400, "usableBytes": 1, "partitions": [entry(1, 50, True), {**entry(7, 25), "partition": "u-7"}]}]},
        {"broker": 2, "logDirs": [{"logDir": "/a", "error": None, "totalBytes": 2000, "usableBytes": 1, "partitions": [entry(0, 90), entry(1, 200)]}]},
        {"broker": 3, "logDirs": [{"logDir": "/a", "error": None, "totalBytes": 700, "usableBytes": 1, "partitions": [entry(1, 180)]},
                                  {"logDir": "/b", "error": None, "partitions": [entry(2, 300)]}]}]}
    return cur, plan, logdirs


def test_stored_bytes_from_both_kinds_of_sizes_document():
    from kafka_assignment_optimizer_amd.waves import parse_pair, parse_sizes, sizes_for, stored_for
    cur, plan, logdirs = _documents()
    wi = parse_pair(cur, plan)
    assert wi.broker_ids.tolist() == [1, 2, 3, 4]
    sizes = parse_sizes(logdirs)
    assert sizes[("t", 0)] == 100 and sizes[("t", 1)] == 200 and sizes[("t", 2)] == 300
    size = sizes_for(wi, sizes)
    assert size.tolist() == [100, 200, 300]
    # a plain sizes document: the sizes of the current rows that hold the broker
    assert stored_for(wi, size).tolist() == [100 + 300, 100 + 200, 200 + 300, 0]
    # kafka-log-dirs: all entries of the broker, future ones included, when that is more (broker 1: 100 + 290 + 50 + 25 = 465)
    assert stored_for(wi, size, logdirs).tolist() == [465, 300, 500, 0]
    assert stored_for(wi, size, json.dumps(logdirs)).tolist() == [465, 300, 500, 0]


def test_capacity_sources_in_order_and_the_missing_ones_named():
    from kafka_assignment_optimizer_amd.waves import capacity_for, parse_pair
    cur, plan, logdirs = _documents()
    wi = parse_pair(cur, plan)
    # an entry first, then totalBytes when every dir reports one (brokers 1, 2; not 3), then the default
    raw, eff = capacity_for(wi, {2: "1K", 9: 5}, logdirs, 5000, 100)
    assert raw.tolist() == [1000, 1024, 5000, 5000] and eff.tolist() == raw.tolist()
    raw, eff = capacity_for(wi, {1: 999, 3: 10, 4: 11}, logdirs, None, 80)
    assert raw.tolist() == [999, 2000, 10, 11] and eff.tolist() == [799, 1600, 8, 8]
    with pytest.raises(ValueError, match=r"no capacity for brokers 3, 4 \("):
        capacity_for(wi, {}, logdirs)
    with pytest.raises(ValueError, match="no capacity for brokers 1, 2, 3, 4"):
        capacity_for(wi, None, None)
    plain = {"partitions": [{"topic": "t", "partition": p, "size": 5} for p in range(3)]}
    with pytest.raises(ValueError, match="no capacity for brokers 1, 2, 3, 4"):
        capacity_for(wi, {}, plain)
    for bad in (0, 101, -5, 50.0, True, "80"):
        with pytest.raises(ValueError, match="max_utilisation must be an integer 1..100"):
            capacity_for(wi, {}, logdirs, 1, bad)
    with pytest.raises(ValueError, match="not a byte count"):
        capacity_for(wi, {1: "12Q"}, logdirs, 1)


def test_plan_waves_reports_a_broker_without_capacity_before_any_device_is_used():
    from kafka_assignment_optimizer_amd.waves import plan_waves
    cur, plan, logdirs = _documents()
    with pytest.raises(ValueError, match="no capacity for brokers 3, 4"):
        plan_waves(cur, plan, sizes=logdirs, headroom=True)
    with pytest.raises(ValueError, match="max_utilisation"):
        plan_waves(cur, plan, sizes=logdirs, default_capacity=10, max_utilisation=0)


def _tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    return [os.path.join(ROOT, "cli", "kao-waves")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.waves"]


def test_both_tools_refuse_misuse_of_the_new_flags(tmp_path):
    base = ["--current", "c.json", "--plan", "p.json", "--out-prefix", "w"]
    for tool in _tools():
        def run(*args):
            return subprocess.run(tool + base + list(args), capture_output=True, cwd=ROOT)
        for flags in (["--headroom"], ["--capacities", "1:5"], ["--default-capacity", "1G"], ["--max-utilisation", "80"]):
            r = run(*flags)
            assert r.returncode == 2 and b"--headroom needs --sizes" in r.stderr, (tool, flags, r.stderr)
        for pct in ("0", "101", "-1", "x", "7.5"):
            assert run("--sizes", "s.json", "--max-utilisation", pct).returncode == 2, (tool, pct)
        assert run("--sizes", "s.json", "--default-capacity", "12Q").returncode == 2
        assert run("--sizes", "s.json", "--headroom", "--max-per-broker", "-1").returncode == 2
        # accepted without any cap: the run gets as far as the documents
        r = run("--sizes", "s.json", "--headroom")
        assert r.returncode == 1, (tool, r.stderr)
        h = subprocess.run(tool + ["--help"], capture_output=True, cwd=ROOT)
        for flag in (b"--headroom", b"--capacities", b"--default-capacity", b"--max-utilisation"):
            assert flag in h.stdout + h.stderr, (tool, flag)


def test_both_tools_name_the_brokers_without_a_capacity(tmp_path):
    cur, plan, logdirs = _documents()
    for name, doc in (("c.json", cur), ("p.json", plan), ("s.json", logdirs)):
        (tmp_path / name).write_text(json.dumps(doc))
    args = ["--current", str(tmp_path / "c.json"), "--plan", str(tmp_path / "p.json"), "--sizes", str(tmp_path / "s.json"), "--out-prefix",
            str(tmp_path / "w"), "--headroom"]
    for tool in _tools():
        r = subprocess.run(tool + args, capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"no capacity for brokers 3, 4 (" in r.stderr, (tool, r.stderr)
        r = subprocess.run(tool + args + ["--capacities", "3:1K,4:12Q"], capture_output=True, cwd=ROOT)
        assert r.returncode == 1 and b"not a byte count" in r.stderr, (tool, r.stderr)
    assert not list(tmp_path.glob("w*"))
