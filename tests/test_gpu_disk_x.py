"""kao_balance_disk_exchange on the MI355X: every instance is held bit for bit against the restatement of the
two kinds of round in tests/disk_x_ref.py: the rows, every number, stats[0..2] and [4..11]; peak_after is never above
kao_balance_disk's on the same device; two calls give the same bytes and dry_run the same numbers."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import disk_ref as dr
import disk_x_ref as dx
from conftest import ROOT
from disk_launches import disk_launches

pytestmark = pytest.mark.gpu
NONE = 0xFFFF


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
    return res.status, res.n_moved, res.bytes_moved, res.peak_before, res.peak_after, res.lower_bound


def _checked(call, c, cap=None, move_leaders=None, min_gain=0, max_rounds=0, ref=None, twice=True):
    """One instance through the GPU against the restatement.  Returns (result, restatement)."""
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    rows = np.asarray(rows, dtype=np.int64)
    cap = c.get("cap", 0) if cap is None else cap
    ml = c.get("move_leaders", True) if move_leaders is None else move_leaders
    if ref is None:
        ref = dx.descend(rows, size, B, rack_of, R, cap, ml, min_gain, max_rounds)
    res = call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, exchange=True)
    plain = call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds)
    print(f"B={B} P={len(rows)} cap={cap} leaders={ml} gpu={_numbers(res)} stats={res.stats.tolist()} plain peak={plain.peak_after}")
    assert res.rows.astype(np.int64).tobytes() == ref["rows"].tobytes()
    assert _numbers(res)[1:5] == (ref["n_moved"], ref["bytes_moved"], ref["peak_before"], ref["peak_after"])
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[4:].tolist() == [ref["rows_changed"], int(ref["more"]), dr.lower_bound(rows, size, B, ml)[1], ref["brokers_changed"], ref["x_rounds"],
                                      ref["exchanges"], ref["x_proposals"], ref["x_peak"]]
    assert (res.exchange_rounds, res.exchanges, res.exchange_proposals, res.peak_of_moves) == tuple(res.stats[8:].tolist())
    assert res.lower_bound == dr.lower_bound(rows, size, B, ml)[0] <= res.peak_after <= plain.peak_after <= res.peak_before
    assert res.status == ("OPTIMAL_PROVEN" if res.peak_after == res.lower_bound else "FEASIBLE_BOUND_GAP")
    if max_rounds == 0:
        assert res.stats[11] == plain.peak_after                       # what the plain call ends at
    if res.stats[8] == 0:
        assert res.rows.tobytes() == plain.rows.tobytes() and _numbers(res) == _numbers(plain) and res.stats[[0, 1, 2, 4, 6, 7]].tolist() == plain.stats[[0, 1, 2, 4, 6, 7]].tolist()
    if twice:
        again = call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, exchange=True)
        dry = call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, dry_run=True, exchange=True)
        assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
        assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()
    return res, ref


@functools.lru_cache(maxsize=None)
def _mid():
    c = dict(dr.lognormal_case(10, 2, 200, 3, 0.7, 7), cap=0, move_leaders=True)
    return c, dx.run(c)


# ---- 1. the small family -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_gain", [0, 5])
def test_small_family_matches_the_restatement(call, min_gain):
    lower = xch = 0
    for seed in range(120):
        res, ref = _checked(call, dr.small_case(seed), min_gain=min_gain, twice=seed % 8 == 0)
        lower += res.peak_after < res.stats[11]
        xch += int(res.stats[9])
    print(f"min_gain={min_gain}: strictly lower than the moves alone: {lower} of 120, exchanges: {xch}")
    if min_gain == 0:
        assert (lower, xch) == (49, 253)   # tests/test_disk_x_ref.py pins the same from the restatement


# ---- 2. the edges of a mask word -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [63, 64, 65, 129])
def test_mask_word_edges(call, N):
    """N positive sizes on three brokers, two replicas each; then the same with zero sizes inside PI's partitions (the positions of
    PI then differ from the partition indices)."""
    rng = np.random.default_rng(N)
    c = dict(rows=np.stack([rng.permutation(3)[:2] for _ in range(N)]).astype(np.int64), size=rng.integers(1, 1000, N), B=3, rack_of=np.zeros(3, dtype=np.int64), R=1)
    res, _ = _checked(call, c)
    assert res.stats[9] > 0
    M = N + 40
    at = np.sort(rng.permutation(M)[:N])
    rows = np.stack([rng.permutation(3)[:2] for _ in range(M)]).astype(np.int64)
    size = np.zeros(M, dtype=np.int64)
    rows[at], size[at] = c["rows"], c["size"]
    holes, _ = _checked(call, dict(c, rows=rows, size=size))
    assert (holes.rows[at] == res.rows).all() and (holes.rows[size == 0] == rows[size == 0]).all() and holes.stats[8:].tolist() == res.stats[8:].tolist()


# ---- 3. widths, padding, racks -------------------------------------------------------------------------------------------------------
def test_width_1_width_8_and_padded_rows(call):
    moved, _ = _checked(call, dx.leaders_only_case())
    assert moved.stats[9] == 1
    kept, _ = _checked(call, dx.leaders_only_case(), move_leaders=False)
    assert kept.n_moved == 0 and kept.stats[0] == 0 and kept.stats[11] == 29
    rng = np.random.default_rng(8)
    c = dict(rows=dr.skewed_rows(rng, 20, 50, 8, pad=0.6), size=rng.integers(1, 1000, 50), B=20, rack_of=np.arange(20) % 4, R=4)   # width 8, mixed k_p
    assert len({int(k) for k in (c["rows"] != NONE).sum(axis=1)}) >= 5
    for cap, ml in ((0, True), (2, True), (2, False)):
        res, _ = _checked(call, c, cap=cap, move_leaders=ml)
        assert res.stats[9] > 0
        assert ((res.rows == NONE) == (c["rows"] == NONE)).all() and (ml or (res.rows[:, 0] == c["rows"][:, 0]).all())
        assert dr.rack_rule_holds(c["rows"], res.rows.astype(np.int64), c["rack_of"], 4, cap)


def test_rack_cases_and_the_hand_built_cases(call):
    rng = np.random.default_rng(3)
    B, R, P = 12, 3, 40
    rack_of = np.arange(B) % R
    rows = np.stack([rng.permutation(R) + R * rng.integers(0, 2, R) for _ in range(P)]).astype(np.int64)   # one replica per rack
    c = dict(rows=rows, size=rng.integers(1, 100, P), B=B, rack_of=rack_of, R=R)
    res, _ = _checked(call, c, cap=1)
    out = res.rows.astype(np.int64)
    assert res.stats[9] > 0 and (rack_of[out] == rack_of[rows]).all()   # every move and every exchange stays inside its rack
    _checked(call, dict(c, rack_of=np.zeros(B, dtype=np.int64), R=1), cap=1)   # one rack, cap 1, width 3: the rows start over the cap
    capped, _ = _checked(call, dx.rack_partner_case())
    assert capped.rows.tolist() == [[2, 1], [2, 1], [3, 0], [0, NONE], [3, NONE]]
    free, _ = _checked(call, dx.rack_partner_case(), cap=0)
    assert free.rows.tolist() == [[2, 1], [2, 0], [3, 1], [0, NONE], [3, NONE]]
    one, ref = _checked(call, dx.shared_partner_case(), max_rounds=1)
    assert ref["shared"] == 1 and one.stats[9] == 1 and one.stats[10] == 2 and one.rows[2].tolist() == [4, 2, 0] and one.rows[1].tolist() == [4, 1, 3]
    full, _ = _checked(call, dx.shared_partner_case())
    assert full.stats[8] == 2 and full.stats[9] == 2
    tight, _ = _checked(call, dx.narrow_gain_case(), min_gain=5)   # 2 min_gain >= D: only y8, before the split of M, passes
    assert tight.rows.tolist() == [[2, 1], [2, 0], [2, 1], [2, 1], [0, NONE]]
    loose, _ = _checked(call, dx.narrow_gain_case())
    assert loose.rows.tolist() == [[2, 1], [2, 1], [2, 1], [2, 0], [0, NONE]]


# ---- 4. equal sizes, contention ------------------------------------------------------------------------------------------------------
def test_equal_sizes_get_the_plain_calls_bytes_and_crowded_cases_match(call):
    for P in (64, 257):
        res, _ = _checked(call, dr.crowded_case(5, P))                  # size 5 everywhere
        assert res.stats[8:11].tolist() == [0, 0, 0] and res.n_moved > 0   # (_checked holds it against the plain call's bytes)
    for seed in (0, 10, 20):
        res, _ = _checked(call, dr.small_case(seed))
        assert res.stats[8:11].tolist() == [0, 0, 0]
    for B, P in ((4, 64), (9, 130)):
        res, _ = _checked(call, dr.crowded_case(B, P, base=2 ** 40))    # the loads pass 2^46
        assert res.n_moved > 0 and res.peak_before > 2 ** 46


# ---- 5. several workgroups, both kinds of round --------------------------------------------------------------------------------------
def test_mid_instance_matches_the_restatement(call):
    """lognormal_case(30, 3, 400, 3, 0.7, 7) with cap 1: two workgroups, 279 rounds of which 197 are exchange rounds, the kinds
    interleaved.  The 3,000 partitions of the same family take the pure-Python restatement seven minutes (3,539 rounds, 2,578 of them exchange
    rounds); 400 is the largest of 400 / 600 / 3,000 it does in under ten seconds.  The 3,000 instance is run for its invariants and
    its counts, which the restatement gave once."""
    c = dr.lognormal_case(30, 3, 400, 3, 0.7, 7)
    res, ref = _checked(call, c, cap=1, twice=False)
    assert "mx" in ref["kinds"] and "xm" in ref["kinds"] and res.stats[8] > 100 and res.stats[3] >= 4 * ref["rounds"]
    assert res.peak_after < res.stats[11] < res.peak_before
    big = dr.lognormal_case(30, 3, 3000, 3, 0.7, 7)
    rows, size = big["rows"], big["size"]
    res = call(rows, 30, big["rack_of"], 3, size, 1, exchange=True)
    plain = call(rows, 30, big["rack_of"], 3, size, 1)
    out = res.rows.astype(np.int64)
    assert (int(res.stats[0]), int(res.stats[8]), int(res.stats[9])) == (3539, 2578, 3083) and res.stats[11] == plain.peak_after
    assert res.peak_after == int(dr.loads(out, size, 30).max()) <= plain.peak_after and (res.n_moved, res.bytes_moved) == dr.set_moves(rows, out, size)
    assert dr.rack_rule_holds(rows, out, big["rack_of"], 3, 1) and dr.stable(out, size, 30, big["rack_of"], 3, 1)
    assert all(len(set(r)) == len(r) for r in out.tolist())


# ---- 6. large sizes, min_gain, max_rounds --------------------------------------------------------------------------------------------
def test_sizes_near_2_to_60_and_the_values_of_min_gain(call):
    rng = np.random.default_rng(60)
    P = 24
    c = dict(rows=np.stack([rng.permutation(6)[:2] for _ in range(P)]).astype(np.int64), size=2 ** 55 + rng.integers(0, 2 ** 54, P), B=6,
             rack_of=np.arange(6) % 2, R=2)   # 48 replicas of up to 1.5 * 2^55: the sum stays below 2^62, the loads pass 2^58
    res, _ = _checked(call, c)
    assert res.stats[9] > 0 and res.peak_before > 2 ** 58
    top = dict(rows=np.array([[0], [0], [1], [1]]), size=np.array([2 ** 60, 2 ** 59, 2 ** 59 + 2 ** 58, 5]), B=2, rack_of=[0, 0], R=1)   # one size of 2^60
    res, _ = _checked(call, top)
    assert res.peak_before == 2 ** 60 + 2 ** 59
    c2, full = _mid()
    D = full["x_peak"] - int(dr.loads(c2["rows"], c2["size"], c2["B"]).min())   # above every gap of the move-stable state
    for mg in (D // 2 + 1, D, 2 ** 62, 2 ** 64 - 1):
        res, ref = _checked(call, c2, min_gain=mg, twice=False)
        assert mg < 2 ** 62 or (res.n_moved == 0 and res.stats[0] == 0 and res.stats[11] == res.peak_before)
    small = dx.narrow_gain_case()
    for mg in (0, 4, 5, 6, 7):   # D = 8: below, at and above D / 2
        _checked(call, small, min_gain=mg)


def test_max_rounds_edges(call):
    c, full = _mid()
    kinds = full["kinds"]
    first_x = kinds.index("x")
    res, _ = _checked(call, c, ref=full, twice=False)
    assert res.stats[5] == 0
    early, _ = _checked(call, c, max_rounds=first_x - 3, twice=False)         # before the first exchange round: the plain call's bytes at that max_rounds
    assert early.stats[5] == 1 and early.stats[8] == 0 and early.stats[11] == 0
    edge, _ = _checked(call, c, max_rounds=first_x, twice=False)              # the probe is the first exchange round
    assert edge.stats[5] == 1 and edge.stats[8] == 0 and edge.stats[11] == full["x_peak"]
    mid, _ = _checked(call, c, max_rounds=len(kinds) - 20)                    # between two exchange rounds
    assert mid.stats[5] == 1 and 0 < mid.stats[8] < full["x_rounds"]
    last, _ = _checked(call, c, max_rounds=len(kinds), ref=full, twice=False)   # exactly at the end: nothing is left, so nothing was stopped (tests/test_disk_x_ref.py)
    assert last.stats[5] == 0 and last.rows.tobytes() == res.rows.tobytes()
    for mr in (32, first_x + 1):                                         # the ends of a batch of rounds
        _checked(call, c, max_rounds=mr, twice=False)


def test_two_calls_in_a_row_leak_no_index_state(call):
    """A larger call, then a smaller one with other sizes, then the first again: each matches its restatement and its first run."""
    a = dr.lognormal_case(12, 3, 150, 3, 0.7, 2)
    b = dx.narrow_gain_case()
    ra = dx.run(a, cap=1)
    first, _ = _checked(call, a, cap=1, ref=ra, twice=False)
    _checked(call, b, twice=False)
    _checked(call, dr.small_case(7), twice=False)
    again, _ = _checked(call, a, cap=1, ref=ra, twice=False)
    assert first.rows.tobytes() == again.rows.tobytes() and first.stats.tolist() == again.stats.tolist()
    empty = call(np.zeros((0, 3)), 4, [0, 1, 0, 1], 2, np.zeros(0, dtype=np.int64), exchange=True)   # no partition
    assert _numbers(empty) == ("OPTIMAL_PROVEN", 0, 0, 0, 0, 0) and empty.stats[[0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]].tolist() == [0] * 11
    zeros, _ = _checked(call, dict(dr.small_case(7), size=np.zeros(len(dr.small_case(7)["rows"]), dtype=np.int64)))   # nothing weighs anything: PI is empty
    assert zeros.stats[0] == 0 and zeros.stats[11] == 0


def test_invalid_arguments_leave_the_rows_alone(kao):
    """Every refusal of include/kao.h is one on a machine with a device too."""
    import test_disk_errors as shared
    import test_disk_x_errors as host
    for what, change, code, text in shared.REFUSED:
        rc, msg = host._call(**change)
        assert rc == code and msg.startswith(host.PREFIX) and text in msg, what


# ---- 7. the command-line tools and the Python API ------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"])


def test_cli_and_python_api_end_to_end(kao, tmp_path):
    """cli/kao-disk --exchange and the Python twin on a two-topic document: the same bytes, the plan the library's, the report line ends
    in the peak of the moves alone and the exchange counts; kao-waves takes the plan as it is."""
    from kafka_assignment_optimizer_amd.disk import balance_disk
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(7)
    B, ids = 9, [100 + 3 * i for i in range(9)]
    racks = {b: f"r{i % 3}" for i, b in enumerate(ids)}
    doc, logdirs = {"version": 1, "partitions": []}, {}
    for name, P, rf in (("alpha", 30, 3), ("be-ta", 20, 2)):
        for p in range(P):
            r = rng.permutation(4)[:rf] if rng.random() < 0.8 else rng.permutation(B)[:rf]   # brokers 0..3 hold most of it
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in r]})
            w = int(rng.integers(1, 1000))
            for b in r:
                logdirs.setdefault(ids[b], []).append({"partition": f"{name}-{p}", "size": w * 1024, "offsetLag": 0, "isFuture": False})
    cur_path, racks_path, sizes_path = (tmp_path / n for n in ("current.json", "racks.json", "logdirs.txt"))
    cur_path.write_text(json.dumps(doc))
    racks_path.write_text(json.dumps({str(b): r for b, r in racks.items()}))
    sizes_path.write_text("Querying brokers for log directories information\n" + json.dumps(
        {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": "/d", "error": None, "partitions": e}]} for b, e in sorted(logdirs.items())]}) + "\n")
    base = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path), "--sizes", str(sizes_path), "--exchange"]
    for tag, flags, kw in (("plain", [], {}), ("rack", ["--max-per-rack", "1", "--keep-leaders", "--min-gain", "1K"], dict(max_per_rack=1, move_leaders=False, min_gain=1024)),
                           ("dry", ["--dry-run"], dict(dry_run=True))):
        outs = []
        for i, prog in enumerate(PROGS):
            out = tmp_path / f"{tag}{i}.json"
            r = subprocess.run(prog + base + flags + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT)
            assert r.returncode == 0, r.stderr
            outs.append((out.read_bytes(), r.stderr.decode()))
        assert outs[0] == outs[1]
        plan, report = json.loads(outs[0][0]), outs[0][1].splitlines()
        lib = balance_disk(doc, sizes_path.read_text(), broker_list=ids, racks=racks, exchange=True, **kw)
        res = lib.result
        both = balance_disk(doc, sizes_path.read_text(), broker_list=ids, racks=racks, **kw).result
        assert plan == lib.document and len(plan["partitions"]) == (0 if tag == "dry" else res.stats[4])
        assert len(report) == 1 and report[0].startswith(f"disk: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} lower_bound={res.lower_bound} ")
        assert report[0].endswith(f" peak_of_moves={res.peak_of_moves} exchange_rounds={res.exchange_rounds} exchanges={res.exchanges} "
                                  f"exchange_proposals={res.exchange_proposals}")
        assert res.exchanges > 0 and res.peak_after <= res.peak_of_moves == both.peak_after < res.peak_before
    r = subprocess.run([os.path.join(ROOT, "cli", "kao-waves"), "--current", str(cur_path), "--plan", str(tmp_path / "plain0.json"), "--sizes", str(sizes_path),
                        "--max-bytes-per-broker", "1M", "--out-prefix", str(tmp_path / "wave")], capture_output=True, cwd=ROOT)
    assert r.returncode == 0 and (tmp_path / "wave1.json").exists(), r.stderr


# ---- 8. the ends of a batch of rounds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rounds,rounds,x_rounds,stopped", [(0, 437, 303, 0), (31, 31, 0, 1), (32, 32, 0, 1), (33, 33, 0, 1), (160, 160, 26, 1)])
def test_max_rounds_on_batch_boundaries(call, max_rounds, rounds, x_rounds, stopped):
    """lognormal_case(24, 4, 400, 3, 0.7, 11), one replica per rack: 437 rounds, 303 of them exchange rounds.  max_rounds before, on
    and after the end of the first batch of 32 rounds, and 160, which reaches into the exchange phase (the whole descent has 134 move
    rounds).  stats[8..11] against the restatement, stats[3] against the launch schedule of tests/disk_launches.py."""
    res, ref = _checked(call, dr.lognormal_case(24, 4, 400, 3, 0.7, 11), cap=1, max_rounds=max_rounds, twice=False)
    assert (ref["rounds"], ref["x_rounds"], int(ref["more"])) == (rounds, x_rounds, stopped)
    assert res.stats[8:].tolist() == [ref["x_rounds"], ref["exchanges"], ref["x_proposals"], ref["x_peak"]]
    assert res.stats[3] == disk_launches(rounds, max_rounds, bool(stopped), exchange=True)
