"""kao_failover_order on the MI355X against the host model of its kernels (tests/failover_ref.py kernel_model), bit for bit: WHICH
of the optimal follower orders it returns and the counters of k_fo_solve (the lowest tight global slot id
becomes the predecessor, targets are served in index order, rounds are counted up to and including the first quiet one).  The
instances sit on both sides of every dispatch edge of the kernels (tests/test_flow_paths_ref.py checks that they do, and the model
against HiGHS); the two around the dynamic-LDS opt-in run in a fresh process each, since the opt-in is remembered per process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import failover_ref as fr
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _same_as_model(rows, B, rack_of, R, scope, got_rows, got_scen, got_stats, dry_rows, dry_scen, dry_stats, dry_n):
    after, scen, stats = fr.kernel_model(rows, B, rack_of, scope, R, with_stats=True)
    print(f"B={B} R={R} P={rows.shape[0]} W={rows.shape[1]} scope={scope} gpu={np.asarray(got_stats).tolist()} model={stats}")
    assert np.asarray(got_scen).tolist() == scen.tolist()
    assert (np.asarray(got_rows, dtype=np.int64) == after).all(), np.nonzero((np.asarray(got_rows) != after).any(axis=1))[0][:10]
    assert np.asarray(got_stats)[0:6].tolist() == stats
    assert int(got_stats[7]) == int(scen[:, 0].max())
    assert (np.asarray(dry_rows, dtype=np.int64) == rows).all() and np.asarray(dry_scen).tolist() == scen.tolist()
    assert np.asarray(dry_stats)[0:6].tolist() == stats and int(dry_stats[7]) == int(scen[:, 0].max()) and dry_n == int(scen[:, 4].sum())
    return scen, stats


def _held(kao, rows, B, rack_of, R, scope):
    """One instance through the GPU: rows, the five values of every scenario and stats[0..5, 7] equal the model's; a dry run reports
    the same numbers on untouched rows.  Returns the model's (scen, stats)."""
    from kafka_assignment_optimizer_amd.failover import failover_order_arrays
    rows = np.asarray(rows, dtype=np.int64)
    res = failover_order_arrays(rows, B, rack_of, R, scope)
    dry = failover_order_arrays(rows, B, rack_of, R, scope, dry_run=True)
    assert res.n_reordered == int(res.scen[:, 4].sum())
    return _same_as_model(rows, B, rack_of, R, scope, res.rows, res.scen, res.stats, dry.rows, dry.scen, dry.stats, dry.n_reordered)


def test_small_family_equals_the_model(kao):
    for rows, B, rack_of, R in fr.small_family():
        for scope in (0, 1):
            _held(kao, rows, B, rack_of, R, scope)


@pytest.mark.parametrize("scope", [0, 1])
def test_named_instances_equal_the_model(kao, scope):
    """The two-arc instance, the odd broker count and 300 brokers x 9,000 partitions (300 workgroups; 2,700 slots on 1,024 lanes)."""
    _, stats = _held(kao, *fr.two_arc_instance(), scope)
    assert stats[5] == 2
    _held(kao, *fr.odd_instance(), scope)
    _held(kao, *fr.many_instance(), scope)


@pytest.mark.parametrize("scope", [0, 1])
@pytest.mark.parametrize("n", [256, 257])
def test_lanes_per_workgroup_edge(kao, n, scope):
    """Broker scope: 1,024 slots in the largest scenario (256 lanes) and 1,028 (1,024 lanes).  Rack scope runs both on 1,024."""
    rows, B, rack_of, R = fr.hot_leader_instance(n)
    scen, stats = _held(kao, rows, B, rack_of, R, scope)
    if scope == 0:
        assert int(scen[:, 0].max()) * rows.shape[1] == {256: 1024, 257: 1028}[n]
    assert stats[5] >= 2 and int(scen[:, 4].sum()) > 100   # paths of several arcs, many swaps


@pytest.mark.parametrize("scope", [0, 1])
@pytest.mark.parametrize("B", [64, 65])
def test_bitmap_word_edge(kao, B, scope):
    """Targets at brokers 31, 32 and B - 1 with B % 32 in {0, 1} (bitmap_instance asserts them from the model's phases)."""
    _held(kao, *fr.bitmap_instance(B), scope)


@pytest.mark.parametrize("B", [1024, 1025])
def test_offsets_scan_edge(kao, B):
    """Broker scope with 1,024 and 1,025 scenarios: one and two scenarios per lane of k_fo_offsets; the last scenario has work."""
    rows, B, rack_of, R = fr.limit_instance(B)
    scen, stats = _held(kao, rows, B, rack_of, R, 0)
    assert stats[0] == 40 and scen[B - 1, 0] > 0


CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np
import failover_ref as fr
import kafka_assignment_optimizer_amd as k
from kafka_assignment_optimizer_amd.failover import failover_order_arrays
k.init(0)
rows, B, rack_of, R = fr.limit_instance({B})
res = failover_order_arrays(rows, B, rack_of, R, 0)   # the first launch of k_fo_solve in this process
dry = failover_order_arrays(rows, B, rack_of, R, 0, dry_run=True)
np.savez({out!r}, rows=res.rows, scen=res.scen, stats=res.stats, dry_rows=dry.rows, dry_scen=dry.scen, dry_stats=dry.stats,
         dry_n=dry.n_reordered, n=res.n_reordered)
"""


@pytest.mark.parametrize("B", [3048, 3049])
def test_dynamic_lds_opt_in_edge_in_a_fresh_process(kao, tmp_path, B):
    """16 B + 4 ceil(B / 32) bytes of dynamic LDS: exactly 48 KiB at B = 3048, which the entry point launches without opening the
    kernel, and 16 bytes more at B = 3049, which it opens the kernel for.  A fresh child process each, so that the launch is the
    first of its process whatever ran before; the child writes what it got, the parent compares."""
    assert fr.lds_bytes(B) == {3048: 49152, 3049: 49168}[B]
    out = str(tmp_path / "result.npz")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), B=B, out=out)
    r = subprocess.run([sys.executable, "-c", code], timeout=120, capture_output=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = np.load(out)
    rows, B, rack_of, R = fr.limit_instance(B)
    scen, stats = _same_as_model(rows, B, rack_of, R, 0, got["rows"], got["scen"], got["stats"], got["dry_rows"], got["dry_scen"],
                                 got["dry_stats"], int(got["dry_n"]))
    assert stats[0] == 40 and int(got["n"]) == int(scen[:, 4].sum()) == 57
