"""kao_plan_waves_sized on the MI355X: waves capped by the bytes each broker moves (and optionally by movements).  Every result
is checked by the independent checker of tests/waves_sized_ref.py (coverage, both caps with the oversize rule, wave 0 / -1, no
empty wave, the exact lower bound) and against the sequential first fit of the kernel's order 0; small instances also bit for
bit against the host restatement of all 64 orders and against the exact optimum (HiGHS)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import waves_ref as wr
import waves_sized_ref as sr
from conftest import GOLDEN, ROOT, load_golden

pytestmark = pytest.mark.gpu
GIB = 1 << 30
TIB = 1 << 40
LOG_DIRS = os.path.join(GOLDEN, "readme_log_dirs.txt")


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def _run(cur, tgt, B, size, C, k, seed=1):
    from kafka_assignment_optimizer_amd.waves import plan_waves_sized_arrays
    return plan_waves_sized_arrays(cur, tgt, B, size, C, k, seed)


def _valid(cur, tgt, B, size, C, k, seed=1):
    wave, nw, lb = _run(cur, tgt, B, size, C, k, seed)
    sr.check_sized(cur, tgt, size, C, k, wave, nw, lb)
    assert nw <= sr.first_fit_sized_waves(cur, tgt, size, C, k)
    return wave, nw, lb


def _readme():
    from kafka_assignment_optimizer_amd.waves import parse_pair, parse_sizes, sizes_for
    cur, prop = load_golden("readme_current.json"), load_golden("readme_proposal.json")
    wi = parse_pair(cur, prop)
    return cur, prop, wi, sizes_for(wi, parse_sizes(open(LOG_DIRS).read()))


def test_kat_readme_proposal_with_sizes(kao):
    """The README proposal moves all 10 partitions; partition p is (p + 1) x 100 MiB, and each source sends 2 copies.  A cap of
    3 GiB per broker needs 2 waves (bound 2: proven); 2 GiB needs 3 (bound 2, and 3 is the HiGHS optimum); 1 GiB needs 4."""
    from kafka_assignment_optimizer_amd.waves import plan_waves
    cur, prop, wi, size = _readme()
    for C, k, expect, lb in ((3 * GIB, 0, 2, 2), (2 * GIB, 0, 3, 2), (GIB, 0, 4, 3), (3 * GIB, 1, 4, 3)):
        res = plan_waves(cur, prop, k, sizes=open(LOG_DIRS).read(), max_bytes_per_broker=C)
        sr.check_sized(wi.current, wi.target, size, C, k, res.wave, res.n_waves, res.lower_bound)
        assert (res.n_waves, res.lower_bound, res.optimal) == (expect, lb, expect == lb), (C, k)
        assert res.n_waves == sr.ilp_min_waves_sized(wi.current, wi.target, size, C, k)
        mw, mnw, _ = sr.kernel_model_sized(wi.current, wi.target, size, C, k, 1)
        assert res.wave.tolist() == mw.tolist()
        tmax = max(t for tt in sr.traffic(wi.current, wi.target, size)[2] for t in tt)   # 2 x 1000 MiB: above 1 GiB
        assert len(res.max_broker_bytes) == res.n_waves and max(res.max_broker_bytes) <= max(C, tmax)
        assert sorted((e["partition"], e["replicas"]) for d in res.waves for e in d["partitions"]) == \
            sorted((e["partition"], e["replicas"]) for e in prop["partitions"])


def test_random_small_instances_match_the_model(kao):
    for s in range(40):
        cur, tgt, size, C, k = sr.random_sized_instance(s)
        B = int(max(cur.max(), tgt.max())) + 1
        wave, nw, lb = _valid(cur, tgt, B, size, C, k, seed=s + 1)
        mwave, mnw, mlb = sr.kernel_model_sized(cur, tgt, size, C, k, s + 1)
        assert (wave.tolist(), nw, lb) == (mwave.tolist(), mnw, mlb), s


def test_random_tiny_instances_reach_the_ilp_optimum(kao):
    """Up to 12 changed partitions each: all 16 pinned seeds reach the HiGHS optimum."""
    for s in range(16):
        cur, tgt, size, C, k = sr.random_sized_instance(s, max_changed=12)
        B = int(max(cur.max(), tgt.max())) + 1
        wave, nw, lb = _valid(cur, tgt, B, size, C, k, seed=s + 1)
        assert nw == sr.ilp_min_waves_sized(cur, tgt, size, C, k), s


def test_oversized_zero_sizes_and_both_caps(kao):
    # one source (broker 0) sends four partitions: 500 (above C), 0, 40 and 70 bytes, each to a broker of its own
    cur = np.array([[0, 1], [0, 2], [0, 3], [0, 4]], dtype=np.uint16)
    tgt = np.array([[0, 5], [0, 6], [0, 7], [0, 8]], dtype=np.uint16)
    size = np.array([500, 0, 40, 70], dtype=np.uint64)
    wave, nw, lb = _valid(cur, tgt, 9, size, 100, 0)
    assert (wave.tolist(), nw, lb) == ([0, 1, 2, 1], 3, 3)   # 500 alone; 70 + 0 ... then 40 (70 + 40 > 100)
    # with a count cap of 1 as well: four waves, the count bound binds
    wave, nw, lb = _valid(cur, tgt, 9, size, 100, 1)
    assert (sorted(wave.tolist()), nw, lb) == ([0, 1, 2, 3], 4, 4)
    # every size 0: the byte cap never binds, the count cap does; a byte cap alone puts everything in one wave
    zero = np.zeros(4, dtype=np.uint64)
    assert _valid(cur, tgt, 9, zero, 1, 2)[1:] == (2, 2)
    assert _valid(cur, tgt, 9, zero, 1, 0)[1:] == (1, 1)
    # nothing changed / only leader order changed
    wave, nw, lb = _run(cur, cur, 9, size, 100, 0)
    assert (wave.tolist(), nw, lb) == ([-1] * 4, 0, 0)
    lead = cur.copy()
    lead[1] = [2, 0]
    wave, nw, lb = _run(cur, lead, 9, size, 100, 0)
    assert (wave.tolist(), nw, lb) == ([-1, 0, -1, -1], 1, 1)


def test_byte_cap_above_every_total_leaves_the_count_cap(kao):
    """C above every T_b: only k binds, and the split is valid for the count-only checker too."""
    for s in range(10):
        cur, tgt, k = wr.random_instance(s)
        k = max(k, 1)
        B = int(max(cur.max(), tgt.max())) + 1
        size = sr.gen_sizes(cur.shape[0], s)
        _, parts, traf = sr.traffic(cur, tgt, size)
        C = max(sr.totals(parts, traf)[0].values(), default=0) + 1
        wave, nw, lb = _valid(cur, tgt, B, size, C, k, seed=s + 1)
        wr.check(cur, tgt, k, wave, nw, lb)


@pytest.mark.parametrize("family", ["config4", "drift100k"])
def test_large_families(kao, family):
    cur, tgt, B = wr.config4_pair() if family == "config4" else wr.drift100k_pair()
    size = sr.gen_sizes(cur.shape[0], 7)
    for C, k in ((4 * TIB, 0), (TIB, 0), (TIB, 2)):
        wave, nw, lb = _valid(cur, tgt, B, size, C, k)
        print(json.dumps({"family": family, "C": C, "k": k, "n_waves": nw, "lower_bound": lb}))


def test_deterministic(kao):
    cur, tgt, B = wr.config4_pair()
    size = sr.gen_sizes(cur.shape[0], 3)
    a = _run(cur, tgt, B, size, TIB, 0, seed=7)
    b = _run(cur, tgt, B, size, TIB, 0, seed=7)
    assert a[0].tolist() == b[0].tolist() and a[1:] == b[1:]


def test_kao_waves_cli_sized_end_to_end(kao, tmp_path):
    """cli/kao-waves with --sizes in both formats (same waves), the bytes report, and the Python twin writing identical files."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    cur_path, plan_path = os.path.join(GOLDEN, "readme_current.json"), os.path.join(GOLDEN, "readme_proposal.json")
    from kafka_assignment_optimizer_amd.waves import parse_sizes
    plain = tmp_path / "sizes.json"
    plain.write_text(json.dumps({"partitions": [{"topic": t, "partition": p, "size": v}
                                                 for (t, p), v in parse_sizes(open(LOG_DIRS).read()).items()]}))
    _, _, wi, size = _readme()
    results = []
    for name, sizes in (("logdirs", LOG_DIRS), ("plain", str(plain))):
        prefix = str(tmp_path / f"cpp_{name}_")
        r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", cur_path, "--plan", plan_path, "--sizes", sizes,
                            "--max-bytes-per-broker", "2G", "--out-prefix", prefix, "--report"], capture_output=True)
        assert r.returncode == 0, r.stderr
        line = r.stderr.decode().strip()
        assert line.startswith("waves=3 lower_bound=2 optimal=no partitions_per_wave="), line
        assert " bytes_lower_bound=2 max_broker_bytes_per_wave=" in line, line
        peaks = [int(v) for v in line.rsplit("=", 1)[1].split(",")]
        assert len(peaks) == 3 and max(peaks) <= 2 * GIB
        docs = [json.load(open(f"{prefix}{w + 1}.json")) for w in range(3)]
        assert not os.path.exists(f"{prefix}4.json")
        results.append((docs, line))
        py = str(tmp_path / f"py_{name}_")
        r2 = subprocess.run([sys.executable, "-m", "kafka_assignment_optimizer_amd.waves", "--current", cur_path, "--plan", plan_path,
                             "--sizes", sizes, "--max-bytes-per-broker", "2G", "--out-prefix", py, "--report"], capture_output=True, cwd=ROOT)
        assert r2.returncode == 0, r2.stderr
        assert r2.stderr.decode().strip() == line
        assert [json.load(open(f"{py}{w + 1}.json")) for w in range(3)] == docs
    assert results[0] == results[1]
    # the waves are the model's
    mw, _, _ = sr.kernel_model_sized(wi.current, wi.target, size, 2 * GIB, 0, 1)
    got = {(e["topic"], e["partition"]): w for w, d in enumerate(results[0][0]) for e in d["partitions"]}
    assert [got[key] for key in wi.keys] == mw.tolist()
    # --default-size sizes the partitions --sizes leaves out; a count cap next to the byte cap
    part = tmp_path / "part.json"
    part.write_text(json.dumps({"partitions": [{"topic": "x.y.z.t", "partition": 9, "size": 5 * GIB}]}))
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", cur_path, "--plan", plan_path, "--sizes", str(part),
                        "--default-size", "1M", "--max-bytes-per-broker", "8G", "--max-per-broker", "2", "--out-prefix",
                        str(tmp_path / "d_"), "--report"], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr.decode().startswith("waves=2 lower_bound=2 optimal=yes"), r.stderr
