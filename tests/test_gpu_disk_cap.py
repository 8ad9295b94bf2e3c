"""kao_balance_disk_capacity on the MI355X: the disk-usage balance by utilisation.  Every case is held byte
for byte against the restatement in tests/disk_cap_ref.py (rows, n_moved, bytes_moved, the peaks and the bound as fractions, the
status, stats[0..2], [4..10]), called twice and once with dry_run, and checked for what holds of every result: the end state is
move-stable by brute force, the rack rule holds, the bytes moved stay inside the budget.  With equal capacities the call is
kao_balance_disk and kao_balance_disk_budget byte for byte."""
import functools
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import disk_cap_ref as cr
import disk_ref as dr
from conftest import ROOT
from disk_launches import disk_launches

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
NO_BUDGET = 2 ** 64 - 1


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@pytest.fixture(scope="module")
def call(kao):
    from kafka_assignment_optimizer_amd.disk import balance_disk_arrays
    return balance_disk_arrays


def _numbers(res):
    return (res.status, res.n_moved, res.bytes_moved, res.peak_before, res.peak_before_capacity, res.peak_after, res.peak_after_capacity, res.lower_bound,
            res.lower_bound_den)


def _reference(c, capacity, max_bytes, cap, ml, min_gain, max_rounds):
    return cr.descend_cap(np.asarray(c["rows"], dtype=np.int64), c["size"], c["B"], c["rack_of"], c["R"], capacity, cap, ml, min_gain, max_rounds, max_bytes)


def _checked(call, c, capacity=None, max_bytes=None, cap=None, move_leaders=None, min_gain=0, max_rounds=0, ref=None):
    """One instance through the GPU against the restatement; max_bytes None = no budget (UINT64_MAX in the call).  Returns (result,
    restatement)."""
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    rows = np.asarray(rows, dtype=np.int64)
    capacity = c["capacity"] if capacity is None else capacity
    cap = c.get("cap", 0) if cap is None else cap
    ml = c.get("move_leaders", True) if move_leaders is None else move_leaders
    ref = _reference(c, capacity, max_bytes, cap, ml, min_gain, max_rounds) if ref is None else ref
    res, again, dry = (call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, dry_run=d, max_bytes=max_bytes, capacity=capacity) for d in (False, False, True))
    print(f"B={B} P={len(rows)} cap={cap} leaders={ml} max_bytes={max_bytes} gpu={_numbers(res)} stats={res.stats.tolist()} ref rounds={ref['rounds']} "
          f"thorough={ref['thorough']} moves={ref['moves']} proposals={ref['proposals']}")
    out = res.rows.astype(np.int64)
    assert len(res.stats) == 11 and res.max_bytes == max_bytes
    assert out.tobytes() == ref["rows"].tobytes()
    bound, _ = cr.lower_bound_cap(rows, size, B, capacity, ml)
    proven, which = cr.proven_cap(ref["peak_after"], rows, size, B, capacity, ml)
    assert _numbers(res) == ("OPTIMAL_PROVEN" if proven else "FEASIBLE_BOUND_GAP", ref["n_moved"], ref["bytes_moved"], *ref["peak_before"], *ref["peak_after"], *bound)
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[4:].tolist() == [ref["rows_changed"], int(ref["more"]), which, ref["brokers_changed"], ref["refused"], int(ref["budget_bound"]), ref["thorough"]]
    # what holds with or without a restatement
    assert (res.n_moved, res.bytes_moved) == dr.set_moves(rows, out, size) and (max_bytes is None or res.bytes_moved <= max_bytes)
    assert (res.peak_after, res.peak_after_capacity) == cr.peak_cap(dr.loads(out, size, B), capacity) and dr.rack_rule_holds(rows, out, rack_of, R, cap)
    assert Fraction(*bound) <= Fraction(res.peak_after, res.peak_after_capacity) <= Fraction(res.peak_before, res.peak_before_capacity)
    assert ((out == NONE) == (rows == NONE)).all() and (ml or (out[:, 0] == rows[:, 0]).all())
    if not ref["more"]:
        if max_bytes is None:
            assert cr.stable_cap(out, size, B, rack_of, R, capacity, cap, ml, min_gain)
        else:
            assert cr.stable_cap(out, size, B, rack_of, R, capacity, cap, ml, min_gain, start=rows, rem=max_bytes - res.bytes_moved)
            assert res.stats[9] == int(not cr.stable_cap(out, size, B, rack_of, R, capacity, cap, ml, min_gain))
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()
    return res, ref


@functools.lru_cache(maxsize=None)
def _small_ref(seed):
    c = cr.small_case_cap(seed)
    return _reference(c, c["capacity"], None, c["cap"], c["move_leaders"], 0, 0)


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
def test_small_family_matches_the_restatement(call):
    thorough = 0
    for seed in range(120):
        res, _ = _checked(call, cr.small_case_cap(seed), ref=_small_ref(seed))
        thorough += res.stats[10] > 0
    assert thorough >= 8


# ---- 2. equal capacities: the byte planners --------------------------------------------------------------------------------------------
def _same_as_plain(call, c, common, max_bytes=None):
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    args = (rows, B, rack_of, R, size, c.get("cap", 0), c.get("move_leaders", True))
    plain = call(*args, max_bytes=max_bytes)
    res = call(*args, max_bytes=max_bytes, capacity=[common] * B)
    assert res.rows.tobytes() == plain.rows.tobytes(), common
    assert (res.n_moved, res.bytes_moved, res.peak_before, res.peak_after, res.status) == (plain.n_moved, plain.bytes_moved, plain.peak_before, plain.peak_after, plain.status)
    assert res.peak_before_capacity == res.peak_after_capacity == common
    keep = [0, 1, 2, 4, 5, 7] + ([] if max_bytes is None else [8, 9])
    assert res.stats[keep].tolist() == plain.stats[keep].tolist() and res.stats[10] == 0 and (max_bytes is not None or res.stats[8:10].tolist() == [0, 0])
    return plain


@pytest.mark.parametrize("common", ["1", "12345", "2^61/B"])
def test_equal_capacities_are_kao_balance_disk(call, common):
    cases = [dr.small_case(seed) for seed in range(120)] + [dr.crowded_case(5, 257)]
    moved = 0
    for c in cases:
        moved += _same_as_plain(call, c, {"1": 1, "12345": 12345}.get(common, 2 ** 61 // c["B"])).n_moved > 0
    assert moved >= 60


def test_equal_capacities_under_a_budget_are_kao_balance_disk_budget(call):
    cases = [dr.small_case(seed) for seed in range(120)] + [dr.crowded_case(5, 257)]
    bound = 0
    for c in cases:
        free = dr.descend(c["rows"], c["size"], c["B"], c["rack_of"], c["R"], c.get("cap", 0), c.get("move_leaders", True))["bytes_moved"]
        bound += int(_same_as_plain(call, c, 12345, max_bytes=free * 3 // 10).stats[9])
    assert bound >= 60


# ---- 3. 128 bits ---------------------------------------------------------------------------------------------------------------------
def test_products_past_64_bits(call):
    """Sizes of 2^40 and a little with capacities near 2^61 / B: every product of a load and a capacity passes 2^64."""
    c = dr.crowded_case(9, 300, base=2 ** 40)
    capacity = [2 ** 61 // 9 - 1000 * b if b % 2 else 2 ** 59 // 9 + 7 * b for b in range(9)]
    assert min(capacity) * int(np.min(c["size"])) > 2 ** 64
    res, ref = _checked(call, c, capacity)
    assert res.n_moved > 0 and ref["rounds"] > 3
    _checked(call, c, capacity, max_bytes=ref["bytes_moved"] // 3)


def _truncated_case():
    """Three brokers, width 1: brokers 0 and 1 hold two partitions each, broker 2 is empty and large.  u(0) > u(1), but with the two
    products cut to 64 bits the comparison goes the other way: the first round's winner would leave broker 1 instead of broker 0."""
    M = 2 ** 64
    for k in range(1, 64):   # the products are near 2^83 and differ by about k 2^62: the cut ones are in the other order for about every other k
        S1 = 3 * 2 ** 30 + 987654321
        S0, c0 = S1 + 1031 * k, 2 ** 52 + 0x9E3779B97F4A7
        c1 = c0 + 1
        if S0 * c1 > S1 * c0 and (S0 * c1) % M < (S1 * c0) % M:
            rows = np.array([[0], [0], [1], [1]])
            size = np.array([S0 - 2 ** 30, 2 ** 30, S1 - 2 ** 30, 2 ** 30], dtype=np.int64)
            return dict(rows=rows, size=size, B=3, rack_of=np.zeros(3, dtype=np.int64), R=1, capacity=[c0, c1, 2 ** 53])
    raise AssertionError("no such instance")


def test_truncated_products_would_change_the_first_winner(call):
    c = _truncated_case()
    S, capv = dr.loads(c["rows"], c["size"], 3), c["capacity"]
    assert cr.ranking_cap(S, capv)[0][0] == 0
    assert (int(S[0]) * capv[1]) % 2 ** 64 < (int(S[1]) * capv[0]) % 2 ** 64   # cut to 64 bits broker 1 would rank first, and the lowest key is the fullest source's
    res, ref = _checked(call, c, max_rounds=1)
    assert ref["moves"] == 1 and res.rows[:, 0].tolist() == [2, 0, 1, 1]   # the winner leaves broker 0
    _checked(call, c)


# ---- 4. thorough rounds --------------------------------------------------------------------------------------------------------------
def test_thorough_rounds(call):
    seeds = [s for s in range(120) if _small_ref(s)["thorough"] > 0]
    assert len(seeds) >= 8
    for seed in seeds:
        res, _ = _checked(call, cr.small_case_cap(seed), ref=_small_ref(seed))
        assert res.stats[10] > 0 and res.stats[0] > res.stats[10]


@pytest.mark.parametrize("P,base,fast,thorough", [(60, 100, 48, 2), (77, 0, 63, 1)], ids=["mid-batch", "last-of-batch"])
def test_first_empty_fast_round_inside_a_batch(call, P, base, fast, thorough):
    """Crowded sources, six brokers with capacities 4 : 1, more than 32 rounds: the first FAST round without a proposal is round
    `fast` (counted from 0), in the middle of the second batch of 32 rounds or its very last round; THOROUGH rounds follow."""
    c = dr.crowded_case(6, P, base=base)
    res, ref = _checked(call, c, np.where(np.arange(6) % 2 == 0, 4, 1) * 1000)
    assert (ref["rounds"] - ref["thorough"], ref["thorough"]) == (fast, thorough) and res.stats[10] == thorough


# ---- 5. the rest of the surface ------------------------------------------------------------------------------------------------------
def _mixed(B=12, R=3, P=80, seed=2):
    c = dr.lognormal_case(B, R, P, 3, 0.7, seed)
    c["capacity"] = np.where(np.arange(B) % 2 == 0, 4, 1) * 2 ** 32 + np.arange(B)
    return c


def test_racks_leaders_min_gain_and_max_rounds(call):
    c = _mixed()
    res, _ = _checked(call, c, cap=1)
    assert res.n_moved > 0 and dr.rack_rule_holds(c["rows"], res.rows.astype(np.int64), c["rack_of"], c["R"], 1)
    res, _ = _checked(call, c, cap=1, move_leaders=False)                     # term (2) against the restatement
    assert res.n_moved > 0
    heavy = dict(c, rows=np.concatenate([c["rows"], np.array([[1, 3, 5]] * 30)]), size=np.concatenate([c["size"], np.full(30, 2 ** 22)]))
    res, _ = _checked(call, heavy, move_leaders=False)                       # broker 1 (a small one) leads 30 heavy partitions
    assert res.stats[6] == 2
    stored = int((np.asarray(c["size"])[:, None] * (c["rows"] != NONE)).sum())
    for min_gain in (stored, 2 ** 64 - 1):                                    # nothing passes the test
        res, _ = _checked(call, c, cap=1, min_gain=min_gain)
        assert res.n_moved == 0 and res.stats[:3].tolist() == [0, 0, 0] and res.stats[10] == 0
    res, _ = _checked(call, c, cap=1, min_gain=2 ** 18)
    assert res.n_moved > 0
    res, ref = _checked(call, c, cap=1, max_rounds=1)
    assert res.stats[0] == 1 and res.stats[5] == 1 and ref["more"]


def test_budget_on_unequal_capacities(call):
    c = _mixed()
    free = _reference(c, c["capacity"], None, 1, True, 0, 0)["bytes_moved"]
    for tenths in (1, 5):
        res, _ = _checked(call, c, cap=1, max_bytes=free * tenths // 10)
        assert 0 < res.bytes_moved <= free * tenths // 10 and res.stats[9] == 1
    res, _ = _checked(call, c, cap=1, max_bytes=0)
    assert res.n_moved == 0 and res.stats[0] == 0 and (res.rows == c["rows"]).all() and res.stats[9] == 1
    for seed in (4, 26, 49, 67, 109):                                          # seeds with THOROUGH rounds, at half their free bytes
        _checked(call, cr.small_case_cap(seed), max_bytes=_small_ref(seed)["bytes_moved"] // 2)


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------
def test_edge_cases(call):
    res = call(np.zeros((0, 3)), 4, [0, 1, 0, 1], 2, np.zeros(0, dtype=np.int64), capacity=[5, 9, 7, 9])   # no partition
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 0, 5, 0, 5, 0, 9) and res.stats[[0, 1, 2, 4, 5, 6, 7, 8, 9, 10]].tolist() == [0] * 10
    res, _ = _checked(call, dict(rows=np.zeros((5, 1)), size=[3, 0, 4, 1, 9], B=1, rack_of=[0], R=1), [40])   # one broker
    assert _numbers(res) == ("OPTIMAL_PROVEN", 0, 0, 17, 40, 17, 40, 17, 40)
    rng = np.random.default_rng(8)
    c = dict(rows=dr.skewed_rows(rng, 20, 50, 8, pad=0.6), size=rng.integers(1, 1000, 50), B=20, rack_of=np.arange(20) % 4, R=4,
             capacity=np.where(np.arange(20) % 3 == 0, 5000, 1300) + np.arange(20))                          # width 8, mixed k_p
    res, _ = _checked(call, dict(c, size=np.zeros(50, dtype=np.int64)))                                       # nothing weighs anything
    assert res.status == "OPTIMAL_PROVEN" and res.n_moved == 0 and res.stats[0] == 0
    res, _ = _checked(call, c, cap=2)
    assert res.n_moved > 0
    res, _ = _checked(call, c, cap=2, move_leaders=False)
    assert res.n_moved > 0
    B = 8000                                                                                                  # the last index in use
    rows = np.array([[B - 1, 0], [B - 1, 1], [B - 1, 2], [0, 1], [B - 1, B - 2], [5, B - 1]])
    c = dict(rows=rows, size=[900, 800, 700, 600, 500, 400], B=B, rack_of=np.arange(B) % 3, R=3, capacity=np.where(np.arange(B) % 2 == 0, 4000, 1000) + np.arange(B) % 7)
    res, _ = _checked(call, c)
    assert res.n_moved > 0 and (res.rows[:4] != rows[:4]).any()
    c = dict(rows=np.array([[0], [0], [1], [1], [1]]), size=[1, 1, 2 ** 40, 2 ** 40, 7], B=3, rack_of=[0, 0, 0], R=1, capacity=[1, 2 ** 61, 2 ** 60])   # capacity 1 beside 2^61
    res, _ = _checked(call, c)
    assert res.n_moved > 0 and (res.peak_before, res.peak_before_capacity) == (2, 1)


# ---- 7. a mid-size instance ----------------------------------------------------------------------------------------------------------
def test_mid_instance_beats_the_byte_plan(call):
    """60 brokers in 6 racks, 1,500 partitions at RF 3, capacities alternating 4 : 1, one replica per rack: several workgroups of
    partitions, more than two batches of rounds.  The peak utilisation ends below that of kao_balance_disk's plan."""
    c = dr.lognormal_case(60, 6, 1500, 3, 0.7, 11)
    capacity = np.where(np.arange(60) % 2 == 0, 4, 1) * 2 ** 32
    res, ref = _checked(call, c, capacity, cap=1)
    assert ref["rounds"] > 64 and ref["thorough"] > 0
    plain = call(c["rows"], 60, c["rack_of"], 6, c["size"], 1)
    byte_plan = Fraction(*cr.peak_cap(dr.loads(plain.rows.astype(np.int64), c["size"], 60), capacity))
    mine = Fraction(res.peak_after, res.peak_after_capacity)
    print(f"peak utilisation: input {float(Fraction(res.peak_before, res.peak_before_capacity)):.6f} byte plan {float(byte_plan):.6f} this plan {float(mine):.6f}")
    assert mine < byte_plan


# ---- 8. the command-line tools -------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"])


def _both(args, tmp_path, tag):
    """Each tool in a fresh child process: the same --out document and the same report."""
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"{tag}{i}.json"
        r = subprocess.run(prog + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, r.stderr
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    report = outs[0][1].splitlines()
    assert len(report) == 1 and report[0].startswith("disk: status=")
    return json.loads(outs[0][0]), report[0]


def test_cli_end_to_end(kao, tmp_path):
    """cli/kao-disk and the Python twin with --capacities on the README example (20 partitions at RF 2 on brokers 0..19, racks by
    parity) with every odd broker a quarter of the size: the same bytes, the library's plan, the report's tail; a broker without a
    capacity is a usage error; without the flag the output is the byte planner's; kao-waves takes the plan."""
    from kafka_assignment_optimizer_amd.disk import balance_disk, report_lines
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import kao_oracle as ko
    doc = json.loads(ko.README_CURRENT) if isinstance(ko.README_CURRENT, str) else ko.README_CURRENT
    ids = list(range(20))
    racks = {b: ("a" if b % 2 == 0 else "b") for b in ids}
    sizes = {"partitions": [{"topic": e["topic"], "partition": e["partition"], "size": (37 * e["partition"] % 11 + 3) * 2 ** 20} for e in doc["partitions"]]}
    caps = {str(b): ("4G" if b % 2 == 0 else 2 ** 30 + b) for b in ids[:-1]}   # broker 19 is left to --default-capacity
    paths = {n: tmp_path / n for n in ("current.json", "racks.json", "sizes.json", "caps.json")}
    for n, d in zip(paths, (doc, {str(b): r for b, r in racks.items()}, sizes, caps)):
        paths[n].write_text(json.dumps(d))
    base = ["--current", str(paths["current.json"]), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(paths["racks.json"]), "--sizes",
            str(paths["sizes.json"]), "--max-per-rack", "1"]
    with_caps = base + ["--capacities", str(paths["caps.json"])]
    for prog in PROGS:   # usage errors exit with 2
        for bad in (with_caps, base + ["--capacities", "0:1G,1:1G"], with_caps + ["--default-capacity", "1X"], base + ["--capacities", "0:abc"]):
            r = subprocess.run(prog + bad + ["--out", str(tmp_path / "x.json")], capture_output=True, cwd=ROOT)
            assert r.returncode == 2 and (bad is not with_caps or b"no capacity for brokers 19 " in r.stderr), (bad, r.stderr)
    kw = dict(broker_list=ids, racks=racks, max_per_rack=1)
    free = balance_disk(doc, sizes, **kw)
    plan, report = _both(base, tmp_path, "free")   # without the flags: today's output, byte for byte
    assert plan == free.document and [report] == report_lines(free) and "_ppm=" not in report and report.endswith(f" launches={free.result.stats[3]}")
    plan, report = _both(with_caps + ["--default-capacity", "4G"], tmp_path, "cap")
    lib = balance_disk(doc, sizes, capacity=caps, default_capacity=4 * 2 ** 30, **kw)
    res = lib.result
    assert plan == lib.document and len(plan["partitions"]) == res.stats[4] > 0 and [report] == report_lines(lib)
    assert report.endswith(f" launches={res.stats[3]} peak_before_ppm={res.peak_before * 10 ** 6 // res.peak_before_capacity} "
                           f"peak_after_ppm={res.peak_after * 10 ** 6 // res.peak_after_capacity} lower_bound_ppm={res.lower_bound * 10 ** 6 // res.lower_bound_den} "
                           f"thorough_rounds={res.stats[10]}")
    assert Fraction(res.peak_after, res.peak_after_capacity) < Fraction(res.peak_before, res.peak_before_capacity)
    plan2, report2 = _both(base + ["--capacities", ",".join(f"{b}:{'4G' if b % 2 == 0 else 2 ** 30 + b}" for b in ids[:-1]), "--default-capacity", "4096M", "--max-bytes", "20M"],
                           tmp_path, "inline")
    capped = balance_disk(doc, sizes, capacity=caps, default_capacity=4 * 2 ** 30, max_bytes=20 * 2 ** 20, **kw)
    assert plan2 == capped.document and [report2] == report_lines(capped) and " budget_bound=" in report2 and capped.result.bytes_moved <= 20 * 2 ** 20
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", str(paths["current.json"]), "--plan", str(tmp_path / "cap0.json"), "--sizes",
                        str(paths["sizes.json"]), "--max-bytes-per-broker", "64M", "--out-prefix", str(tmp_path / "wave")], capture_output=True, cwd=ROOT)
    assert r.returncode == 0 and (tmp_path / "wave1.json").exists(), r.stderr


# ---- 9. the ends of a batch of rounds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,max_bytes,max_rounds,rounds,thorough,stopped", [
    (50, None, 0, 99, 4, 0), (59, None, 0, 97, 2, 0), (4, None, 0, 130, 0, 0), (50, None, 95, 95, 0, 1), (50, None, 96, 96, 1, 1), (50, None, 97, 97, 2, 1),
    (50, None, 99, 99, 4, 0), (50, None, 100, 99, 4, 0), (50, 3 * 10 ** 8, 0, 51, 0, 0)])
def test_thorough_switch_and_max_rounds_on_batch_boundaries(call, seed, max_bytes, max_rounds, rounds, thorough, stopped):
    """lognormal_case(24, 4, 400, 3, 0.7, seed), one replica per rack, capacities of 1, 2 or 4 MB drawn with the same seed.  Seed 50:
    the first empty FAST round is round 95, the last of a batch of 32, and the 4 THOROUGH rounds fill one batch of 4 exactly.  Seed
    59: 2 THOROUGH rounds.  Seed 4: the switch is followed at once by an empty THOROUGH round.  On seed 50 max_rounds falls on the
    switch, inside the THOROUGH batch, on its end (the probe finds nothing left) and past it; once more under a budget.  No seed in
    0..119 of this family ends its FAST rounds at an exact multiple of 32.  stats[3] is the launch schedule of tests/disk_launches.py."""
    c = dr.lognormal_case(24, 4, 400, 3, 0.7, seed)
    capacity = np.random.default_rng(seed).choice([1, 2, 4], 24) * 10 ** 6
    res, ref = _checked(call, c, capacity, max_bytes=max_bytes, cap=1, max_rounds=max_rounds)
    assert (ref["rounds"], ref["thorough"], int(ref["more"])) == (rounds, thorough, stopped)
    assert res.stats[3] == disk_launches(rounds, max_rounds, bool(stopped), budget=max_bytes is not None, capacity=True, thorough=thorough)
