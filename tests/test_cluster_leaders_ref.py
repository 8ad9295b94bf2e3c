"""CPU tests of the cluster-wide leader balance (kao_balance_leaders_cluster): the HiGHS reference of
tests/cluster_leaders_ref.py against enumeration on tiny instances, the mix of the small family the GPU tests rely on, the host
restatement of the kernels' probes and phases against the reference; the entry point is declared, exported and bound, rejects bad
input before touching a device and fails loudly without one; the command-line tools' usage errors."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cluster_leaders_ref as cr
from conftest import ROOT, have_gpu

NONE = 0xFFFF
SEEDS = range(80)


@pytest.fixture(autouse=True, scope="module")
def bound():
    """The reference restates an entry point: without it there is nothing to hold it against."""
    from kafka_assignment_optimizer_amd import _ffi
    assert "kao_balance_leaders_cluster" in _ffi.SIGNATURES
    return _ffi.load().kao_balance_leaders_cluster


@pytest.fixture(scope="module")
def small():
    """seed -> (case, optimum, optimum with every topic band opened to [0, P])"""
    out = {}
    for seed in SEEDS:
        case = rows, topic_of, B, LO, tlo, thi = cr.small_case(seed)
        P = len(rows)
        out[seed] = (case, cr.optimum(*case), cr.optimum(rows, topic_of, B, LO, np.zeros_like(tlo), np.full_like(thi, P)))
    return out


def test_optimum_equals_enumeration_on_tiny_instances():
    feasible = 0
    for seed in range(40):
        case = cr.tiny_case(seed)
        assert len(case[0]) <= 8
        opt = cr.optimum(*case)
        assert opt == cr.enumerate_all(*case), seed
        feasible += opt is not None
    assert 10 <= feasible <= 35, feasible   # both verdicts occur


def test_small_family_has_the_mix_the_gpu_tests_need(small):
    """A condition on the inputs, not on the code under test."""
    feasible = sum(opt is not None for _, opt, _ in small.values())
    bands_bind = sum(opt is not None and opt != free for _, opt, free in small.values())
    lower = sum(opt is not None and opt[0] < int(np.bincount(case[0][:, 0], minlength=case[2]).max()) for case, opt, _ in small.values())
    print(f"feasible={feasible} infeasible={len(small) - feasible} bands_bind={bands_bind} peak_lower={lower}")
    assert feasible >= 50 and len(small) - feasible >= 15 and bands_bind >= 30 and lower >= 40


def test_kernel_model_matches_the_reference(small):
    """The kernels' schedule on the host: verdict, peak and changes equal the LP's, the rows are swaps that meet every band; a fixed
    cap one above the optimum gives that LP's changes, one below is infeasible."""
    for seed, (case, opt, _) in small.items():
        rows, topic_of, B, LO, tlo, thi = case
        ok, out, n, before, after, stats = cr.kernel_model(*case)
        assert before == int(np.bincount(rows[:, 0], minlength=B).max())
        assert stats[6] == len({(t, b) for t, r in zip(topic_of.tolist(), rows.tolist()) for b in r if b != NONE})
        if opt is None:
            assert not ok and n == 0 and after == before and (out == rows).all(), seed
            continue
        assert ok and (after, n) == opt and stats[7] == 0, (seed, opt, after, n)
        assert cr.check_rows(rows, out) == n and cr.admissible(out, topic_of, B, LO, after, tlo, thi), seed
        ok, out, n, _, peak, _ = cr.kernel_model(*case, cluster_hi=after + 1)
        assert ok and n == cr.lp(rows, topic_of, B, LO, after + 1, tlo, thi) and peak <= after + 1, seed
        assert cr.admissible(out, topic_of, B, LO, after + 1, tlo, thi), seed
        if after - 1 >= LO:
            assert not cr.kernel_model(*case, cluster_hi=after - 1)[0], seed


def test_mid_instance_reference():
    """mid_case(100, 20, 150, 3, 0) at topic bands [0, 3]: the model against the two LPs around its peak; the topic bands bind."""
    rows, topic_of = cr.mid_case(100, 20, 150, 3, 0)
    tlo, thi = np.zeros(20, dtype=np.int64), np.full(20, 3)
    ok, out, n, before, after, stats = cr.kernel_model(rows, topic_of, 100, 0, tlo, thi)
    assert ok and cr.lp(rows, topic_of, 100, 0, after - 1, tlo, thi) is None and cr.lp(rows, topic_of, 100, 0, after, tlo, thi) == n
    assert cr.lp(rows, topic_of, 100, 0, after, tlo, np.full(20, 3000)) < n
    assert cr.check_rows(rows, out) == n and cr.admissible(out, topic_of, 100, 0, after, tlo, thi) and after < before


# ---- the entry point ---------------------------------------------------------------------------------------------------------------
def _call(rows, B, topic_of, tlo, thi, clo=0, chi=-1, null=None, P=None, W=None, T=None):
    from kafka_assignment_optimizer_amd import _ffi
    r = np.ascontiguousarray(rows, dtype=np.uint16)
    keep = r.copy()
    tof = np.ascontiguousarray(topic_of, dtype=np.int32)
    lo, hi = np.ascontiguousarray(tlo, dtype=np.int32), np.ascontiguousarray(thi, dtype=np.int32)
    out = [C.c_int32(0) for _ in range(4)]
    i32 = C.POINTER(C.c_int32)
    args = [B, r.shape[0] if P is None else P, r.shape[1] if W is None else W, r.ctypes.data_as(C.POINTER(C.c_uint16)), tof.ctypes.data_as(i32),
            len(lo) if T is None else T, lo.ctypes.data_as(i32), hi.ctypes.data_as(i32), clo, chi, 0] + [C.byref(o) for o in out] + [None]
    if null is not None:
        args[null] = None
    rc = _ffi.load().kao_balance_leaders_cluster(*args)
    assert (r == keep).all()   # a rejected call leaves the rows alone
    return rc


def test_entry_point_is_declared_exported_and_bound(bound):
    from kafka_assignment_optimizer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "kao.h")).read()
    assert re.search(r"\bint kao_balance_leaders_cluster\(int32_t n_brokers, int32_t n_partitions, int32_t width,\s+"
                     r"uint16_t \*rows /\* \[n_partitions\*width\] in / out \*/,\s+"
                     r"const int32_t \*topic_of /\* \[n_partitions\], 0\.\.n_topics-1 \*/, int32_t n_topics,\s+"
                     r"const int32_t \*topic_lo, const int32_t \*topic_hi /\* \[n_topics\] \*/,\s+"
                     r"int32_t cluster_lo, int32_t cluster_hi /\* -1 = minimise the peak \*/, int32_t dry_run,\s+"
                     r"int32_t \*n_changed, int32_t \*peak_before, int32_t \*peak_after, int32_t \*status,\s+"
                     r"int32_t stats\[8\] /\* may be NULL \*/\);", header)
    assert "#define KAO_VERSION 103" in header
    res, args = _ffi.SIGNATURES["kao_balance_leaders_cluster"]
    P = C.POINTER
    assert res is C.c_int
    assert args == [C.c_int32, C.c_int32, C.c_int32, P(C.c_uint16), P(C.c_int32), C.c_int32, P(C.c_int32), P(C.c_int32), C.c_int32, C.c_int32,
                    C.c_int32, P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_int32)]
    assert bound.argtypes == args and bound.restype is C.c_int


INVALID = [
    ("null rows", dict(null=3)), ("null topic_of", dict(null=4)), ("null topic_lo", dict(null=6)), ("null topic_hi", dict(null=7)),
    ("null n_changed", dict(null=11)), ("null peak_before", dict(null=12)), ("null peak_after", dict(null=13)), ("null status", dict(null=14)),
    ("width 0", dict(W=0)), ("width above KAO_MAX_RF", dict(W=9)), ("no broker", dict(B=0)), ("too many brokers", dict(B=65535)),
    ("negative partitions", dict(P=-1)), ("no topic", dict(T=0)), ("topic_of above", dict(topic_of=[0, 2, 1])),
    ("topic_of below", dict(topic_of=[0, -1, 1])), ("topic_lo negative", dict(tlo=[-1, 0])), ("topic_lo above topic_hi", dict(tlo=[0, 2])),
    ("cluster_lo negative", dict(clo=-1)), ("cluster_hi below -1", dict(chi=-2)), ("cluster_hi below cluster_lo", dict(clo=2, chi=1)),
    ("slot 0 empty", dict(rows=[[0, 1], [NONE, 3], [1, 2]])), ("a broker after an empty slot", dict(rows=[[0, NONE, 1], [2, 3, NONE], [1, 2, 0]])),
    ("index >= n_brokers", dict(rows=[[0, 1], [2, 4], [1, 2]])), ("broker twice", dict(rows=[[0, 1], [3, 3], [1, 2]])),
]


@pytest.mark.parametrize("what,change", INVALID, ids=[w for w, _ in INVALID])
def test_entry_point_rejects_bad_input(what, change):
    """KAO_ERR_INVALID (-1), checked on the host before any device is used; the rows stay as they are."""
    kw = dict(rows=[[0, 1], [2, 3], [1, 2]], B=4, topic_of=[0, 0, 1], tlo=[0, 0], thi=[1, 1])
    kw.update(change)
    assert _call(**kw) == -1


def test_entry_point_reports_unsupported_sizes():
    rows = np.zeros((1, 2), dtype=np.uint16)
    assert _call(rows, 4, [0], [0], [1], P=2000001) == -2   # more than 4,000,000 slots: KAO_ERR_UNSUPPORTED, before a row is read


@pytest.mark.skipif(have_gpu(), reason="checks the no-device failure mode")
def test_fails_loudly_without_gpu():
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_cluster_arrays
    rows = np.array([[0, 1], [0, 2], [1, 2]])
    assert _call(rows, 3, [0, 0, 1], [0, 0], [2, 2]) == -3   # KAO_ERR_NO_DEVICE
    with pytest.raises(kao.KaoError) as e:
        balance_leaders_cluster_arrays(rows, 3, [0, 0, 1], [0, 0], [2, 2])
    assert e.value.code == -3


def test_python_front_end_checks_its_arguments():
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders_cluster, balance_leaders_cluster_arrays
    with pytest.raises(ValueError, match="rows"):
        balance_leaders_cluster_arrays(np.zeros(4), 3, [0], [0], [1])
    with pytest.raises(ValueError, match="topic_of"):
        balance_leaders_cluster_arrays(np.zeros((2, 2)), 3, [0], [0], [1])
    with pytest.raises(ValueError, match="no topic"):
        balance_leaders_cluster([])
    a = Topic(name="a", broker_ids=np.arange(3), rack_of=np.zeros(3), n_racks=1, n_partitions=2, rf=2, current=np.array([[0, 1], [1, 2]]))
    b = Topic(name="b", broker_ids=np.arange(4), rack_of=np.zeros(4), n_racks=1, n_partitions=2, rf=2, current=np.array([[0, 1], [1, 2]]))
    with pytest.raises(ValueError, match="share one broker index"):
        balance_leaders_cluster([a, b])
    with pytest.raises(ValueError, match="distinct"):
        balance_leaders_cluster([a, a])


def test_cli_usage_errors(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    base = ["--current", str(tmp_path / "c.json"), "--broker-list", "0,1,2", "--racks", "0:a,1:b,2:a"]
    for prog in ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"]):
        for extra in (["--cluster", "--auto-slack"], ["--cluster-hi", "3", "--auto-slack"], ["--cluster", "--cluster-lo", "-1"],
                      ["--cluster-lo", "2", "--cluster-hi", "1"], ["--cluster-lo", "1"], ["--cluster-hi"]):
            r = subprocess.run(prog + base + extra, capture_output=True, cwd=ROOT)
            assert r.returncode == 2, (prog, extra, r.stderr)
        r = subprocess.run(prog + base + ["--cluster"], capture_output=True, cwd=ROOT)   # the document does not exist
        assert r.returncode == 1, (prog, r.stderr)
    cur = tmp_path / "c.json"
    cur.write_text('{"version":1,"partitions":[{"topic":"a","partition":0,"replicas":[0,1]},{"topic":"b","partition":7,"replicas":[2,5,1]}]}')
    for prog in ([os.path.join(ROOT, "cli", "kao-leaders")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.leaders"]):
        r = subprocess.run(prog + base + ["--cluster"], capture_output=True, cwd=ROOT)   # broker 5 is outside the list
        assert r.returncode == 1 and b"b-7" in r.stderr and b"broker 5" in r.stderr, (prog, r.stderr)
