"""kao_balance_disk_banded on the MI355X: disk-usage balance inside a replica-count band, with and without
exchange rounds.  Every instance is held byte for byte against the restatement of the rounds in tests/disk_band_ref.py: rows, all
numbers, count_range, stats[0..2] and [4..13]; every case runs twice and once with dry_run, and is checked for the invariants: no count
leaves [min(lo, n0), max(hi, n0)], no move inside the band is left, the rack rule holds.  With a band no count reaches the call is
kao_balance_disk or kao_balance_disk_exchange, launch for launch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import disk_band_ref as db
import disk_ref as dr
import disk_x_ref as dx
from conftest import ROOT

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
    return res.status, res.n_moved, res.bytes_moved, res.peak_before, res.peak_after, res.lower_bound, res.count_range, res.outside_band, res.outside_band_before


def _checked(call, c, band, exchange=False, cap=None, move_leaders=None, min_gain=0, max_rounds=0):
    """One instance through the GPU against the restatement: bytes, numbers, count_range, stats[0..2] and [4..13]; twice, and once with
    dry_run; every invariant.  Returns (result, restatement)."""
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    rows = np.asarray(rows, dtype=np.int64)
    size = np.asarray(size, dtype=np.int64)
    cap = c.get("cap", 0) if cap is None else cap
    ml = c.get("move_leaders", True) if move_leaders is None else move_leaders
    ref = db.descend_band(rows, size, B, rack_of, R, band, cap, ml, min_gain, max_rounds, exchange)
    res, again, dry = (call(rows, B, rack_of, R, size, cap, ml, min_gain, max_rounds, dry_run=d, exchange=exchange, count_band=band) for d in (False, False, True))
    print(f"B={B} P={len(rows)} band={band} exchange={exchange} cap={cap} leaders={ml} gpu={_numbers(res)} stats={res.stats.tolist()} ref rounds={ref['rounds']} "
          f"moves={ref['moves']} proposals={ref['proposals']} exchanges={ref['exchanges']}")
    out = res.rows.astype(np.int64)
    assert out.tobytes() == ref["rows"].tobytes()
    bound, term = dr.lower_bound(rows, size, B, ml)
    assert _numbers(res)[1:] == (ref["n_moved"], ref["bytes_moved"], ref["peak_before"], ref["peak_after"], bound, ref["count_range"], ref["outside_after"],
                                 ref["outside_before"])
    assert res.status == ("OPTIMAL_PROVEN" if ref["peak_after"] == bound else "FEASIBLE_BOUND_GAP")
    assert res.stats[:3].tolist() == [ref["rounds"], ref["moves"], ref["proposals"]]
    assert res.stats[4:].tolist() == [ref["rows_changed"], int(ref["more"]), term, ref["brokers_changed"], ref["x_rounds"], ref["exchanges"], ref["x_proposals"],
                                      ref["x_peak"], ref["outside_after"], ref["outside_before"]]
    assert res.count_band == (band[0], min(band[1], 2 ** 31 - 1))
    # what holds with or without a restatement
    n0, n = db.counts(rows, B), db.counts(out, B)
    assert res.count_range == (int(n0.min()), int(n0.max()), int(n.min()), int(n.max()))
    assert (n >= np.minimum(band[0], n0)).all() and (n <= np.maximum(band[1], n0)).all()
    assert (res.outside_band, res.outside_band_before) == (db.outside(n, band), db.outside(n0, band)) and res.outside_band <= res.outside_band_before
    assert res.peak_after == int(dr.loads(out, size, B).max(initial=0)) <= res.peak_before == int(dr.loads(rows, size, B).max(initial=0))
    assert (res.n_moved, res.bytes_moved) == dr.set_moves(rows, out, size) and dr.rack_rule_holds(rows, out, rack_of, R, cap)
    assert ((out == NONE) == (rows == NONE)).all() and (ml or not len(rows) or (out[:, 0] == rows[:, 0]).all())
    if not ref["more"]:
        assert db.stable_band(out, size, B, rack_of, R, band, cap, ml, min_gain) and res.lower_bound <= res.peak_after
        assert not exchange or len(rows) > 400 or dx.exchange_stable(out, size, B, rack_of, R, cap, ml, min_gain)
    assert res.rows.tobytes() == again.rows.tobytes() and _numbers(res) == _numbers(again) and res.stats.tolist() == again.stats.tolist()
    assert _numbers(dry) == _numbers(res) and (dry.rows == rows).all() and dry.stats.tolist() == res.stats.tolist()
    return res, ref


# ---- 1. the small family ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
def test_small_family_matches_the_restatement(call, exchange):
    moved = bound_by_band = 0
    for seed in range(120):
        c = dr.small_case(seed)
        band = db.band_of(seed, db.counts(c["rows"], c["B"]))
        res, _ = _checked(call, c, band, exchange)
        moved += res.stats[1] > 0
        bound_by_band += res.outside_band_before > 0
    print(f"moved: {moved} of 120, a broker outside the band at the start: {bound_by_band}")
    assert moved >= 60 and bound_by_band >= 20


# ---- 2. a band no count reaches: the calls without a band ----------------------------------------------------------------------------------
def _same_as_unbanded(call, c, cap, ml, exchange, **kw):
    rows, size, B, rack_of, R = (c[k] for k in ("rows", "size", "B", "rack_of", "R"))
    plain = call(rows, B, rack_of, R, size, cap, ml, exchange=exchange, **kw)
    res = call(rows, B, rack_of, R, size, cap, ml, exchange=exchange, count_band=(0, len(rows)), **kw)
    assert res.rows.tobytes() == plain.rows.tobytes()
    assert _numbers(res)[:6] == (plain.status, plain.n_moved, plain.bytes_moved, plain.peak_before, plain.peak_after, plain.lower_bound)
    assert res.stats[:8].tolist() == plain.stats[:8].tolist()   # the launch count among them: the counts are built inside the call's own launches
    assert res.stats[8:12].tolist() == (plain.stats[8:].tolist() if exchange else [0] * 4) and res.stats[12:].tolist() == [0, 0]
    return res


@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
def test_a_band_no_count_reaches_is_the_call_without_a_band(call, exchange):
    moved = 0
    for seed in range(120):
        c = dr.small_case(seed)
        moved += _same_as_unbanded(call, c, c["cap"], c["move_leaders"], exchange).n_moved > 0
        _same_as_unbanded(call, c, c["cap"], c["move_leaders"], exchange, max_rounds=2, min_gain=3)
    assert moved >= 60
    for ml in (True, False):
        assert _same_as_unbanded(call, dr.lognormal_case(60, 6, 1500, 3, 0.7, 5), 1, ml, exchange, max_rounds=0 if not exchange else 120).n_moved > 0


# ---- 3. two and three brokers, width 1 ---------------------------------------------------------------------------------------------------
def _one_rack(rows, size, B):
    return dict(rows=np.array(rows), size=np.array(size, dtype=np.int64), B=B, rack_of=np.zeros(B, dtype=np.int64), R=1)


@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
def test_two_brokers_the_only_destination_is_full(call, exchange):
    c = _one_rack([[0], [0], [0], [1]], [5, 3, 4, 1], 2)
    res, _ = _checked(call, c, (0, 1), exchange)                # n(1) = 1 = hi: nothing arrives there
    assert res.stats[1] == (1 if exchange else 0) and (res.n_moved == 0) == (not exchange) and res.count_range == (1, 3, 1, 3)
    free, _ = _checked(call, c, (0, 2), exchange)
    assert free.stats[1] >= 1 and free.count_range[2:] == (2, 2)


@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
def test_three_brokers_the_only_source_is_at_the_floor(call, exchange):
    c = _one_rack([[0], [0], [0], [1], [2]], [5, 3, 4, 1, 1], 3)
    res, _ = _checked(call, c, (3, 9), exchange)                # n(0) = 3 = lo: nothing leaves it; brokers 1 and 2 are below lo and may receive
    assert (res.n_moved == 0) == (not exchange) and res.outside_band_before == 2 and res.count_range[:2] == (1, 3)
    free, _ = _checked(call, c, (2, 9), exchange)
    assert free.stats[1] >= 1 and free.count_range[3] == 2


# ---- 4. the widest rows, some padded -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
def test_width_8_with_padded_rows(call, exchange):
    rng = np.random.default_rng(11)
    c = dict(dr.lognormal_case(12, 3, 40, 8, 0.9, 3), cap=3)
    cut = rng.integers(2, 9, 40)
    c["rows"][np.arange(8)[None, :] >= cut[:, None]] = NONE
    n0 = db.counts(c["rows"], 12)
    for band in ((int(n0.min()), int(n0.max())), (int(n0.mean()), int(n0.mean()) + 1), (0, 40)):
        _checked(call, c, band, exchange)


# ---- 5. either side of the 256-lane workgroup edge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
@pytest.mark.parametrize("P", [255, 256, 257])
def test_partition_count_around_the_workgroup_edge(call, P, exchange):
    c = dr.lognormal_case(6, 2, P, 2, 0.7, P)
    total = 2 * P
    res, ref = _checked(call, c, (total // 6 - 2, -(-total // 6) + 2), exchange, max_rounds=40 if exchange else 0)
    assert res.stats[1] > 0 and res.rows[P - 1].tolist() != [NONE, NONE]


# ---- 6. two sources aimed at one destination with one place left ---------------------------------------------------------------------------------
def test_two_sources_one_destination_with_one_place_left(call):
    """Brokers 0 and 1 are heavy, broker 2 is light with n = hi - 1, broker 3 is full and light: both sources propose to broker 2, one
    wins a round; in the next round broker 2 is full.  Every intermediate state is compared: no round overfills."""
    c = _one_rack([[0], [0], [0], [1], [1], [1], [2], [3], [3]], [9, 8, 7, 9, 8, 6, 1, 1, 1], 4)
    band = (0, 2)
    seen = []
    for max_rounds in range(1, 6):
        res, ref = _checked(call, c, band, max_rounds=max_rounds)
        assert db.counts(res.rows, 4).max() <= 3 and db.counts(res.rows, 4)[2] <= 2 and db.counts(res.rows, 4)[3] <= 2
        seen.append(res.rows.tobytes())
        if not ref["more"]:
            break
    assert not ref["more"] and ref["rounds"] >= 1 and db.counts(res.rows, 4)[2] == 2 and len(set(seen)) >= 1
    first, _ = _checked(call, c, band, max_rounds=1)
    assert first.stats[2] >= 2 and first.stats[1] == 1          # two proposals into broker 2, one winner


# ---- 7. every source far above hi, every destination below lo -------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
def test_crowded_case(call, exchange):
    c = dr.crowded_case(9, 100)                                 # 100 replicas on each of brokers 0..2, none on 3..8
    res, _ = _checked(call, c, (30, 36), exchange)
    assert res.outside_band_before == 9 and res.count_range[:2] == (0, 100) and res.count_range[3] < 100 and res.stats[1] > 0
    res, _ = _checked(call, dr.crowded_case(9, 100, base=1000), (33, 34), exchange)
    assert res.stats[1] > 0


# ---- 8. an exact band on a count-balanced start ------------------------------------------------------------------------------------------------
def test_exact_band_on_a_balanced_start(call):
    c = db.balanced_case(6, 60, 3, 0.7, 1)
    res, _ = _checked(call, c, (30, 30))
    assert res.stats[0] == 0 and res.n_moved == 0 and (res.rows == c["rows"]).all() and res.peak_after == res.peak_before
    both, _ = _checked(call, c, (30, 30), exchange=True)
    assert both.count_range == (30, 30, 30, 30) and both.exchanges > 0 and both.stats[1] == both.exchanges and both.peak_after < both.peak_before
    wider = db.balanced_case(12, 200, 3, 0.7, 2, R=3)
    n0 = db.counts(wider["rows"], 12)
    assert n0.tolist() == [50] * 12
    both, _ = _checked(call, wider, (50, 50), exchange=True, cap=1)
    assert both.count_range == (50, 50, 50, 50) and both.peak_after < both.peak_before


# ---- 9. the leaders kept, one replica per rack ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", [False, True], ids=["moves", "exchange"])
def test_leaders_kept_and_one_replica_per_rack(call, exchange):
    c = dr.lognormal_case(12, 4, 120, 3, 0.7, 8)
    for ml, cap in ((False, 0), (True, 1), (False, 1)):
        res, _ = _checked(call, c, (27, 33), exchange, cap=cap, move_leaders=ml)
        assert res.stats[1] > 0


# ---- 10. the mid instance ----------------------------------------------------------------------------------------------------------------------
def test_mid_instance_matches_the_restatement(call):
    """60 brokers in 6 racks, 1,500 partitions at RF 3, slack 2 around the mean of 75: several workgroups and several batches of
    rounds.  Moves only: the restatement of the exchange rounds takes minutes at this size, and the small cases above cover them."""
    c = dr.lognormal_case(60, 6, 1500, 3, 0.7, 5)
    res, ref = _checked(call, c, (73, 77), cap=1)
    assert ref["rounds"] > 32 and res.outside_band_before > 30 and res.outside_band < res.outside_band_before


# ---- 11. the command-line tools ---------------------------------------------------------------------------------------------------------
PROGS = ([os.path.join(ROOT, "cli", "kao-disk")], [sys.executable, "-m", "kafka_assignment_optimizer_amd.disk"])


def test_cli_end_to_end(kao, tmp_path):
    """cli/kao-disk --count-slack 1 --exchange and the Python twin on a two-topic document over nine brokers in three racks: the same
    plan, the same report; the report's band line is the library's numbers."""
    from kafka_assignment_optimizer_amd.disk import balance_disk
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    rng = np.random.default_rng(9)
    ids = [100 + 3 * i for i in range(9)]
    racks = {b: f"r{i % 3}" for i, b in enumerate(ids)}
    doc, sizes = {"version": 1, "partitions": []}, {"partitions": []}
    for name, P, rf in (("alpha", 14, 3), ("be-ta", 9, 2)):
        for p in range(P):
            doc["partitions"].append({"topic": name, "partition": p, "replicas": [ids[b] for b in rng.permutation(9)[:rf]]})
            sizes["partitions"].append({"topic": name, "partition": p, "size": int(rng.integers(1, 1000)) * 1024})
    cur_path, racks_path, sizes_path = (tmp_path / n for n in ("current.json", "racks.json", "sizes.json"))
    cur_path.write_text(json.dumps(doc))
    racks_path.write_text(json.dumps({str(b): r for b, r in racks.items()}))
    sizes_path.write_text(json.dumps(sizes))
    args = ["--current", str(cur_path), "--broker-list", ",".join(str(b) for b in ids), "--racks", str(racks_path), "--sizes", str(sizes_path),
            "--count-slack", "1", "--exchange", "--max-per-rack", "2", "--report"]
    outs = []
    for i, prog in enumerate(PROGS):
        out = tmp_path / f"plan{i}.json"
        r = subprocess.run(prog + args + ["--out", str(out)], capture_output=True, cwd=ROOT)
        assert r.returncode == 0, (prog, r.returncode, r.stderr)
        outs.append((out.read_bytes(), r.stderr.decode()))
    assert outs[0] == outs[1]
    plan, report = json.loads(outs[0][0]), outs[0][1].splitlines()
    lib = balance_disk(doc, sizes, broker_list=ids, racks=racks, max_per_rack=2, exchange=True, count_slack=1)
    res = lib.result
    assert plan == lib.document and res.count_band == (60 // 9 - 1, -(-60 // 9) + 1) == (5, 8) and res.stats[1] > 0
    assert report[0].startswith(f"disk: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} lower_bound={res.lower_bound} ")
    assert report[0].endswith(f" peak_of_moves={res.peak_of_moves} exchange_rounds={res.exchange_rounds} exchanges={res.exchanges} exchange_proposals={res.exchange_proposals}")
    r = res.count_range
    assert report[1] == f"disk: replica_band=5:8 counts_before={r[0]}..{r[1]} counts_after={r[2]}..{r[3]} outside_before={res.outside_band_before} outside_after={res.outside_band}"
    assert len(report) == 2 + (res.outside_band > 0) and (not res.outside_band or report[2].startswith(f"kao-disk: warning: {res.outside_band} brokers"))
