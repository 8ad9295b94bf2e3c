"""CPU tests of the byte-capped wave planner's host layer (kao_plan_waves_sized, waves.parse_sizes, the new kao-waves flags): the
entry point is declared, exported and bound, rejects bad input before touching a device, fails loudly without one; sizes are read
from `kafka-log-dirs --describe` output and from a plain document; the reference is consistent on hand cases."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import waves_sized_ref as sr
from conftest import GOLDEN, ROOT, have_gpu, load_golden

NONE = 0xFFFF
LOG_DIRS = os.path.join(GOLDEN, "readme_log_dirs.txt")


def _call(B, cur, tgt, size, cap, k, null_size=False):
    from kafka_assignment_optimizer_amd import _ffi
    cur = np.ascontiguousarray(cur, dtype=np.uint16)
    tgt = np.ascontiguousarray(tgt, dtype=np.uint16)
    sz = np.ascontiguousarray(size, dtype=np.uint64)
    P = cur.shape[0]
    wave = np.zeros(max(P, 1), dtype=np.int32)
    nw, lb = C.c_int32(0), C.c_int32(0)
    u16, u64, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    return _ffi.load().kao_plan_waves_sized(B, P, cur.shape[1], cur.ctypes.data_as(u16), tgt.ctypes.data_as(u16),
                                            None if null_size else sz.ctypes.data_as(u64), cap, k, 1, wave.ctypes.data_as(i32),
                                            C.byref(nw), C.byref(lb))


def test_plan_waves_sized_is_declared_exported_and_bound():
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_plan_waves_sized\(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t \*current,\s+"
                     r"const uint16_t \*target,\s+const uint64_t \*size /\* \[n_partitions\] bytes \*/, uint64_t max_bytes_per_broker,\s+"
                     r"int32_t max_per_broker,\s+uint64_t seed, int32_t \*wave /\* \[n_partitions\] \*/, int32_t \*n_waves, "
                     r"int32_t \*lower_bound\);", header)
    res, args = _ffi.SIGNATURES["kao_plan_waves_sized"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [C.c_int32, C.c_int32, C.c_int32, P(C.c_uint16), P(C.c_uint16), P(C.c_uint64), C.c_uint64, C.c_int32, C.c_uint64,
                    P(C.c_int32), P(C.c_int32), P(C.c_int32)]
    fn = _ffi.load().kao_plan_waves_sized
    assert fn.argtypes == args and fn.restype is C.c_int


def test_plan_waves_sized_rejects_bad_input():
    """KAO_ERR_INVALID (-1), checked on the host before any device is used (so also on a machine without one)."""
    cur = np.array([[0, 1], [2, 3]])
    tgt = np.array([[0, 4], [2, 3]])
    size = [10, 20]
    assert _call(5, cur, tgt, size, 100, 1, null_size=True) == -1     # size == NULL
    assert _call(5, cur, tgt, size, 0, 0) == -1                       # no cap at all
    assert _call(5, cur, tgt, size, 100, -1) == -1                    # k < 0
    assert _call(4, cur, tgt, size, 100, 1) == -1                     # the row checks of kao_plan_waves: broker 4 >= n_brokers
    assert _call(5, cur, np.array([[0, 0], [2, 3]]), size, 100, 1) == -1
    # traffic: broker 4 receives 2^62 bytes in all (two partitions of 2^61), the source 0 sends 3 x 2^61 on its own
    cur2 = np.array([[0, 1], [2, 3]])
    tgt2 = np.array([[4, 1], [4, 3]])
    assert _call(5, cur2, tgt2, [1 << 61, 1 << 61], 100, 0) == -1
    assert _call(5, cur2, tgt2, [1 << 61, (1 << 61) - 1], 1, 0) != -1       # just below: accepted
    cur3 = np.array([[0, 1, 2]])
    tgt3 = np.array([[5, 6, 7]])
    assert _call(8, cur3, tgt3, [(1 << 62) // 3 + 1], 1, 0) == -1     # the source sends 3 x size >= 2^62
    assert _call(8, cur3, tgt3, [(1 << 64) - 1], 1, 0) == -1          # n_added x size overflows 64 bits
    # sizes of partitions that move no data are not traffic: no overflow from them
    assert _call(5, cur, cur, [(1 << 64) - 1, (1 << 64) - 1], 1, 0) in (0, -3)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_plan_waves_sized_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd import waves
    assert _call(5, np.array([[0, 1]]), np.array([[0, 4]]), [7], 10, 0) == -3   # KAO_ERR_NO_DEVICE
    with pytest.raises(kao.KaoError) as e:
        waves.plan_waves(load_golden("readme_current.json"), load_golden("readme_proposal.json"), sizes=open(LOG_DIRS).read(),
                         max_bytes_per_broker=1 << 30)
    assert e.value.code == -3


def test_parse_sizes_kafka_log_dirs():
    """The fixture is `kafka-log-dirs --describe` output for the README topic: partition p is (p + 1) x 100 MiB on both of its
    replicas; broker 0 also holds a larger future replica of partition 0, which does not count."""
    from kafka_assignment_optimizer_amd.waves import parse_sizes
    text = open(LOG_DIRS).read()
    got = parse_sizes(text)
    assert got == {("x.y.z.t", p): (p + 1) * 100 * 1024 ** 2 for p in range(10)}
    assert parse_sizes(json.loads(text.splitlines()[-1])) == got          # the JSON line on its own, parsed
    # topic names with '-', the largest non-future replica, a partition with only a future replica is missing
    doc = {"version": 1, "brokers": [
        {"broker": 1, "logDirs": [{"partitions": [{"partition": "my-topic-12", "size": 5, "isFuture": False},
                                                  {"partition": "a-b-0", "size": 70, "isFuture": True}]}]},
        {"broker": 2, "logDirs": [{"partitions": [{"partition": "my-topic-12", "size": 9, "isFuture": False}]},
                                  {"partitions": [{"partition": "my-topic-3", "size": 0, "isFuture": False}]}]}]}
    assert parse_sizes(doc) == {("my-topic", 12): 9, ("my-topic", 3): 0}
    with pytest.raises(ValueError, match="topic"):
        parse_sizes({"brokers": [{"logDirs": [{"partitions": [{"partition": "nodash", "size": 1}]}]}]})
    with pytest.raises(ValueError, match="2\\^53"):
        parse_sizes({"brokers": [{"logDirs": [{"partitions": [{"partition": "t-1", "size": (1 << 53) + 1}]}]}]})
    with pytest.raises(ValueError, match="no JSON"):
        parse_sizes("Querying brokers for log directories information\n")


def test_parse_sizes_plain_document():
    from kafka_assignment_optimizer_amd.waves import parse_sizes
    doc = {"partitions": [{"topic": "t-x", "partition": 3, "size": 123}, {"topic": "u", "partition": 0, "size": 1 << 53}]}
    assert parse_sizes(doc) == {("t-x", 3): 123, ("u", 0): 1 << 53}
    assert parse_sizes(json.dumps(doc)) == parse_sizes(doc)
    for bad in (-1, 1.5, (1 << 53) + 1, "7", True):
        with pytest.raises(ValueError):
            parse_sizes({"partitions": [{"topic": "t", "partition": 0, "size": bad}]})
    with pytest.raises(ValueError, match="twice"):
        parse_sizes({"partitions": [{"topic": "t", "partition": 0, "size": 1}] * 2})
    with pytest.raises(ValueError):
        parse_sizes({"version": 1})


def test_sizes_for_names_missing_moving_partitions():
    from kafka_assignment_optimizer_amd.waves import parse_pair, sizes_for
    wi = parse_pair(load_golden("readme_current.json"), load_golden("readme_proposal.json"))
    with pytest.raises(ValueError, match="x.y.z.t-0, x.y.z.t-1, x.y.z.t-2, x.y.z.t-3, x.y.z.t-4 and 5 more"):
        sizes_for(wi, {})
    assert sizes_for(wi, {("x.y.z.t", 4): 9}, default_size=1).tolist() == [1] * 4 + [9] + [1] * 5
    # a partition the plan leaves unchanged needs no size
    plan = {"version": 1, "partitions": [{"topic": "x.y.z.t", "partition": 1, "replicas": [8, 1]}]}
    wi = parse_pair(load_golden("readme_current.json"), plan)
    assert sizes_for(wi, {("x.y.z.t", 1): 5}).tolist() == [0, 5] + [0] * 8


def test_bytes_code_is_monotone():
    vals = [0, 1, 2, 3, 511, 512, 513, 1023, 1024, 1 << 20, (1 << 20) + 1, (1 << 40) - 1, 1 << 40, (1 << 62) - 1, (1 << 64) - 1]
    codes = [sr.bytes_code(v) for v in vals]
    assert codes == sorted(codes) and codes[0] == 0 and codes[1] == 1 << 9 and max(codes) == (64 << 9 | 511)
    assert sr.bytes_code(1 << 40) == 41 << 9 and sr.bytes_code((1 << 40) + (1 << 39)) == 41 << 9 | 256


def test_reference_on_hand_cases():
    """Traffic, the oversize rule, the lower bounds and the sequential first fit on cases small enough to check by hand."""
    # p0 moves 0 -> 3 (adds 3, source 0), p1 adds 4 and 5 with source 1, p2 only reorders, p3 is unchanged
    cur = np.array([[0, 1], [1, 2], [2, 0], [1, 0]])
    tgt = np.array([[3, 1], [4, 5], [0, 2], [1, 0]])
    size = [100, 30, 7, 9]
    cls, parts, traf = sr.traffic(cur, tgt, size)
    assert cls == [1, 1, 0, -1]
    assert parts[:2] == [[3, 0], [4, 5, 1]] and traf[:2] == [[100, 100], [30, 30, 60]]
    # p0 and p1 share no broker: one wave under any byte cap that fits them, or under a cap below both (each goes alone)
    for C, k in ((100, 0), (1, 0), (50, 1)):
        w, nw, lb = sr.kernel_model_sized(cur, tgt, size, C, k, 1)
        assert (w.tolist(), nw) == ([0, 0, 0, -1], 1)
        sr.check_sized(cur, tgt, size, C, k, w, nw, lb)
    assert sr.lower_bound_sized(cur, tgt, size, 1, 0) == 1          # every participant: one oversized partition, min(t, C) = C
    # one source b = 0 sends three partitions: sizes 60, 50, 40 under C = 100
    cur = np.array([[0, 1], [0, 2], [0, 3]])
    tgt = np.array([[0, 4], [0, 5], [0, 6]])
    size = [60, 50, 40]
    assert sr.lower_bound_sized(cur, tgt, size, 100, 0) == 2        # ceil(150 / 100)
    w, nw, lb = sr.kernel_model_sized(cur, tgt, size, 100, 0, 1)
    assert (w.tolist(), nw, lb) == ([0, 1, 0], 2, 2)                # first fit decreasing: 60 + 40, then 50
    assert sr.ilp_min_waves_sized(cur, tgt, size, 100, 0) == 2
    # the same with a count cap of 1: three waves, and the count bound says so
    w, nw, lb = sr.kernel_model_sized(cur, tgt, size, 100, 1, 1)
    assert (sorted(w.tolist()), nw, lb) == ([0, 1, 2], 3, 3)
    # an oversized partition opens wave 0 alone at broker 0; the 40-byte one and then the empty one (placed after it, so it
    # sees the load of 500 > C) share wave 1.  The byte bound counts the oversized one as C: ceil((100 + 0 + 40) / 100) = 2
    size = [500, 0, 40]
    w, nw, lb = sr.kernel_model_sized(cur, tgt, size, 100, 0, 1)
    assert (w.tolist(), nw, lb) == ([0, 1, 1], 2, 2)
    sr.check_sized(cur, tgt, size, 100, 0, w, nw, lb)
    with pytest.raises(AssertionError):                             # 500 and 40 together at broker 0
        sr.check_sized(cur, tgt, size, 100, 0, [0, 0, 0], 1, 2)


def _cli(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    return subprocess.run([os.path.join(ROOT, "cli", "kao-waves")] + list(args), capture_output=True)


def test_cli_usage_errors_for_the_new_flags():
    base = ["--current", "c.json", "--plan", "p.json", "--out-prefix", "w"]
    assert _cli(*base).returncode == 2                                                   # no cap at all
    assert _cli(*base, "--max-per-broker", "0").returncode == 2                          # as before
    assert _cli(*base, "--max-bytes-per-broker", "0").returncode == 2                    # both caps 0
    assert _cli(*base, "--max-bytes-per-broker", "0", "--max-per-broker", "0").returncode == 2
    assert _cli(*base, "--max-bytes-per-broker", "1G", "--max-per-broker", "-1").returncode == 2
    for bad in ("", "x", "1X", "-5", "1.5G", "16777216T"):
        assert _cli(*base, "--max-bytes-per-broker", bad).returncode == 2, bad
    assert _cli(*base, "--max-bytes-per-broker", "1G", "--default-size", "9007199254740993").returncode == 2
    assert _cli(*base, "--sizes").returncode == 2
    # accepted: the run gets as far as reading the documents
    for ok in (["--max-bytes-per-broker", "1024"], ["--max-bytes-per-broker", "2t"], ["--sizes", "s.json", "--max-per-broker", "2"]):
        r = _cli("--current", "/nonexistent.json", "--plan", "p.json", "--out-prefix", "w", *ok)
        assert r.returncode == 1 and b"cannot open" in r.stderr, (ok, r.stderr)


def test_cli_missing_sizes_and_bad_sizes_are_errors(tmp_path):
    cur, plan = os.path.join(GOLDEN, "readme_current.json"), os.path.join(GOLDEN, "readme_proposal.json")
    sizes = tmp_path / "s.json"
    sizes.write_text(json.dumps({"partitions": [{"topic": "x.y.z.t", "partition": 0, "size": 1}]}))
    r = _cli("--current", cur, "--plan", plan, "--out-prefix", str(tmp_path / "w"), "--sizes", str(sizes), "--max-bytes-per-broker", "1G")
    assert r.returncode == 1 and b"no size for moving partitions x.y.z.t-1, x.y.z.t-2" in r.stderr, r.stderr
    sizes.write_text(json.dumps({"partitions": [{"topic": "x.y.z.t", "partition": 0, "size": 9007199254740993}]}))
    r = _cli("--current", cur, "--plan", plan, "--out-prefix", str(tmp_path / "w"), "--sizes", str(sizes), "--max-bytes-per-broker", "1G")
    assert r.returncode == 1 and b"2^53" in r.stderr, r.stderr
    assert not list(tmp_path.glob("w*.json"))


def test_python_twin_usage_errors(tmp_path):
    def run(*args):
        return subprocess.run([sys.executable, "-m", "kafka_assignment_optimizer_amd.waves"] + list(args), capture_output=True, cwd=ROOT)
    base = ["--current", "c.json", "--plan", "p.json", "--out-prefix", "w"]
    assert run(*base).returncode == 2
    assert run(*base, "--max-bytes-per-broker", "0").returncode == 2
    assert run(*base, "--max-bytes-per-broker", "1Q").returncode == 2
    cur, plan = os.path.join(GOLDEN, "readme_current.json"), os.path.join(GOLDEN, "readme_proposal.json")
    sizes = tmp_path / "s.json"
    sizes.write_text(json.dumps({"partitions": [{"topic": "x.y.z.t", "partition": 0, "size": 1}]}))
    r = run("--current", cur, "--plan", plan, "--out-prefix", str(tmp_path / "w"), "--sizes", str(sizes), "--max-bytes-per-broker", "1G")
    assert r.returncode == 1 and b"no size for moving partitions x.y.z.t-1, x.y.z.t-2" in r.stderr, r.stderr
