"""Times kao_balance_disk on: BASELINE config 4 after a drift with its 200 topics concatenated over the one broker index (500
brokers x 10,000 partitions, its own racks, no rack rule) and the large instance of tests/leaders_ref.py (1000 brokers x 100,000
partitions, RF 3, 10 racks, max_per_rack 1), each with log-normal sizes of sigma 0.7 and 1.5.  One JSON line per case: peaks, lower
bound, peak_after / lower_bound, replicas and bytes moved, the bytes stored, the stats (rounds, moves, proposals, kernel launches)
and the wall time of the call with dry_run (median of --reps after one warm-up; it includes the host validation, the upload and the
read-back of the counters, and ends in a stream synchronise).  For kernel times run it under
`rocprofv3 --kernel-trace --stats --` (in a run of its own, --reps 1).  Writes the lines to profiles/disk_time.txt with --write.
--max-bytes-pct 1,2,5,none times kao_balance_disk_budget instead, once per value: a budget of that share of
the bytes stored, `none` = UINT64_MAX; the lines gain the budget, what is left of it, the refused winners, budget_bound and the time
of every repeat, and --write puts them into profiles/disk_budget_time.txt.
--capacity 4:1 times kao_balance_disk_capacity on the same families with a bimodal capacity vector: even
brokers have 4 * 2^36 bytes of disk, odd ones 2^36.  --capacity equal gives every broker 2^36 (the byte planner's plan: the cost of
the 128-bit rank and test).  The lines gain the peaks and the bound as fractions and in parts per million, the mean utilisation,
the thorough rounds and, for the same instance, the peak utilisation that kao_balance_disk's plan reaches; --write puts them into
profiles/disk_capacity_time.txt.
--exchange times kao_balance_disk and kao_balance_disk_exchange in one process, case by case, each the median
of --reps after a warm-up, with dry_run.  The cases `small` (12 brokers x 1,200 partitions, 3 racks, max_per_rack 1) and `mid` (100 x
10,000, 10 racks, max_per_rack 1) of tests/disk_ref.py's log-normal family may be named in --cases beside the two above.  A line
carries, as plain call -> this call: peak / bound, bytes moved, rounds (move + exchange), launches and wall time, then the exchanges
and the cost of one exchange round against one move round (the extra wall time over the exchange rounds; the plain call's wall time
over its rounds).  --write appends the lines to profiles/disk_x_time.txt.  --max-rounds N caps the rounds of both calls.
--drain N[,N..] times kao_balance_disk and kao_balance_disk_drain in one process on the same rows, the N
heaviest brokers draining, once per N.  A line carries the draining brokers' largest replica count (stats[9] is at least that), the
rounds, drain moves (stats[8]), the last round with a drain move (stats[9]), what is left, peak / bound, bytes moved and, as plain call
-> this call, rounds, launches and wall time.  --write appends the lines to profiles/disk_drain_time.txt.
--band LO:HI|slack=K[,...] times kao_balance_disk (kao_balance_disk_exchange with --exchange) and kao_balance_disk_banded (DESIGN.md
section 4x) in one process on the same rows, once per band.  Its cases are COUNT-BALANCED starts (tests/disk_band_ref.py's
balanced_case: every broker holds the same number of replicas): `balanced500` (500 brokers x 10,000 partitions, RF 3, no rack rule, 60
replicas each) and `balanced1000` (1000 x 100,000, RF 3, 10 racks, max_per_rack 1, 300 each).  slack=K is the band of kao-disk
--count-slack K (slack=0 is the exact band); a band no count reaches, 0:1000000, is the control: its time against the call without a
band is what the band's own loads and stores cost.  A line carries, as call without a band -> banded call: peak / bound, rounds,
moves, exchanges, bytes copied, wall time and microseconds per round with their ratio; and the count range before -> after and the
brokers outside the band.  --write appends the lines to profiles/disk_band_time.txt."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="config4,large")
    ap.add_argument("--sigmas", default="0.7,1.5")
    ap.add_argument("--keep-leaders", action="store_true")
    ap.add_argument("--max-bytes-pct", default=None, help="CSV of budgets in percent of the bytes stored, or `none`: times kao_balance_disk_budget")
    ap.add_argument("--capacity", default=None, choices=["4:1", "equal"], help="times kao_balance_disk_capacity with this capacity vector")
    ap.add_argument("--exchange", action="store_true", help="times kao_balance_disk and kao_balance_disk_exchange side by side")
    ap.add_argument("--drain", default=None, help="CSV of N: times kao_balance_disk and kao_balance_disk_drain side by side, the N heaviest brokers draining")
    ap.add_argument("--band", default=None, help="CSV of LO:HI or slack=K: times the call without a band and kao_balance_disk_banded side by side on count-balanced starts")
    ap.add_argument("--max-rounds", type=int, default=0)
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/disk_time.txt (disk_budget_time.txt with --max-bytes-pct) as well")
    a = ap.parse_args()
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.disk import BUDGET_STAT_KEYS, CAPACITY_STAT_KEYS, STAT_KEYS, balance_disk_arrays
    import leaders_ref as lr
    kao.init(0)

    def sizes(P, sigma, seed):
        rng = np.random.default_rng(seed)
        return np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), sigma, P)))).astype(np.int64)

    def timed(rows, B, rack_of, R, size, cap, max_bytes, capacity=None, exchange=False, drain=None, count_band=None):
        args = (rows, B, rack_of, R, size, cap, not a.keep_leaders, 0, a.max_rounds)
        res = balance_disk_arrays(*args, dry_run=True, max_bytes=max_bytes, capacity=capacity, exchange=exchange, drain=drain, count_band=count_band)   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = balance_disk_arrays(*args, dry_run=True, max_bytes=max_bytes, capacity=capacity, exchange=exchange, drain=drain, count_band=count_band)
            ms.append(round(1e3 * (time.perf_counter() - t0), 3))
        return res, ms

    cases = {}   # name -> rows, B, rack_of, R, max_per_rack
    if a.band is not None:   # count-balanced starts only
        import disk_band_ref as db
        from kafka_assignment_optimizer_amd.disk import slack_band
        for name, (B, P, R, cap) in (("balanced500", (500, 10000, 1, 0)), ("balanced1000", (1000, 100000, 10, 1))):
            if a.cases in ("config4,large", "") or name in a.cases.split(","):
                c = db.balanced_case(B, P, 3, 0.7, 7, R=R)   # (the sizes are drawn per sigma below)
                cases[name] = (c["rows"], B, c["rack_of"].astype(np.uint8), R, cap)
        a.cases = ""
    if "config4" in a.cases:
        topics = lr.config4_topics()
        cases["config4"] = (np.concatenate([np.asarray(t.current, dtype=np.int64) for t in topics]), topics[0].n_brokers,
                            np.asarray(topics[0].rack_of, dtype=np.uint8), topics[0].n_racks, 0)
    if "large" in a.cases:
        rows, B, _, _ = lr.large_instance()
        cases["large"] = (rows, B, (np.arange(B) % 10).astype(np.uint8), 10, 1)
    import disk_ref as dr
    for name, shape in (("small", (12, 3, 1200, 3)), ("mid", (100, 10, 10000, 3))):
        if name in a.cases.split(","):
            c = dr.lognormal_case(*shape, 0.7, 7, zeros=0.0)   # (the sizes are drawn per sigma below)
            cases[name] = (c["rows"], shape[0], c["rack_of"].astype(np.uint8), shape[1], 1)
    lines = []
    for name, (rows, B, rack_of, R, cap) in cases.items():
        for sigma in (float(s) for s in a.sigmas.split(",")):
            size = sizes(len(rows), sigma, 11)
            total = int((size[:, None] * (rows != 0xFFFF)).sum())
            if a.band is not None:
                plain, pms = timed(rows, B, rack_of, R, size, cap, None, exchange=a.exchange)
                pm = float(np.median(pms))
                for text in a.band.split(","):
                    band = slack_band(int((rows != 0xFFFF).sum()), B, int(text[6:])) if text.startswith("slack=") else tuple(int(v) for v in text.split(":"))
                    res, bms = timed(rows, B, rack_of, R, size, cap, None, exchange=a.exchange, count_band=band)
                    bm = float(np.median(bms))
                    lb = max(res.lower_bound, 1)
                    us = [round(1e3 * pm / max(int(plain.stats[0]), 1), 2), round(1e3 * bm / max(int(res.stats[0]), 1), 2)]
                    line = {"workload": name, "sigma": sigma, "brokers": B, "racks": R, "partitions": len(rows), "max_per_rack": cap, "move_leaders": not a.keep_leaders,
                            "max_rounds": a.max_rounds, "exchange": a.exchange, "band": text, "count_band": list(band), "count_range": list(res.count_range),
                            "outside_band": [res.outside_band_before, res.outside_band], "status": res.status, "lower_bound": res.lower_bound, "peak_before": res.peak_before,
                            "peak_after": [plain.peak_after, res.peak_after], "peak_over_bound": [round(plain.peak_after / lb, 5), round(res.peak_after / lb, 5)],
                            "rounds": [int(plain.stats[0]), int(res.stats[0])], "moves": [int(plain.stats[1]), int(res.stats[1])],
                            "exchanges": [int(plain.stats[9]) if a.exchange else 0, int(res.stats[9])], "replicas_moved": [plain.n_moved, res.n_moved],
                            "bytes_moved": [plain.bytes_moved, res.bytes_moved], "gib_moved": [round(plain.bytes_moved / 2 ** 30, 2), round(res.bytes_moved / 2 ** 30, 2)],
                            "bytes_total": total, "launches": [int(plain.stats[3]), int(res.stats[3])], "stopped_by_max_rounds": [int(plain.stats[5]), int(res.stats[5])],
                            "wall_ms_median": [round(pm, 3), round(bm, 3)], "wall_ms": [pms, bms], "us_per_round": us,
                            "us_per_round_ratio": round(us[1] / us[0], 3) if us[0] and int(res.stats[0]) else None}
                    lines.append(json.dumps(line))
                    print(lines[-1], flush=True)
                    if a.write:
                        with open(os.path.join(ROOT, "profiles", "disk_band_time.txt"), "a") as f:
                            f.write(lines[-1] + "\n")
                continue
            if a.drain is not None:
                plain, pms = timed(rows, B, rack_of, R, size, cap, None)
                S = np.zeros(B, dtype=np.int64)
                held = rows != 0xFFFF
                np.add.at(S, rows[held], np.broadcast_to(size[:, None], rows.shape)[held])
                for n in (int(x) for x in a.drain.split(",")):
                    ids = np.lexsort((np.arange(B), -S))[:n]   # the n heaviest, the lower index on ties
                    flags = np.zeros(B, dtype=np.uint8)
                    flags[ids] = 1
                    res, dms = timed(rows, B, rack_of, R, size, cap, None, drain=flags)
                    pm, dm = float(np.median(pms)), float(np.median(dms))
                    lb = max(res.lower_bound, 1)
                    line = {"workload": name, "sigma": sigma, "brokers": B, "racks": R, "partitions": len(rows), "max_per_rack": cap, "move_leaders": not a.keep_leaders,
                            "max_rounds": a.max_rounds, "draining": n, "drain_ids": [int(b) for b in ids], "drain_replicas_max": int(max((rows == b).sum() for b in ids)),
                            "drain_replicas": int(sum((rows == b).sum() for b in ids)), "status": res.status, "rounds": [int(plain.stats[0]), int(res.stats[0])],
                            "drain_moves": res.drain_moves, "last_drain_round": res.last_drain_round, "replicas_left": res.n_left, "bytes_left": res.bytes_left,
                            "peak_before": res.peak_before, "peak_after": [plain.peak_after, res.peak_after], "lower_bound": [plain.lower_bound, res.lower_bound],
                            "peak_over_bound": [round(plain.peak_after / max(plain.lower_bound, 1), 5), round(res.peak_after / lb, 5)],
                            "replicas_moved": [plain.n_moved, res.n_moved], "bytes_moved": [plain.bytes_moved, res.bytes_moved], "bytes_total": total,
                            "moves": [int(plain.stats[1]), int(res.stats[1])], "launches": [int(plain.stats[3]), int(res.stats[3])],
                            "stopped_by_max_rounds": [int(plain.stats[5]), int(res.stats[5])], "wall_ms_median": [round(pm, 3), round(dm, 3)], "wall_ms": [pms, dms]}
                    lines.append(json.dumps(line))
                    print(lines[-1], flush=True)
                    if a.write:
                        with open(os.path.join(ROOT, "profiles", "disk_drain_time.txt"), "a") as f:
                            f.write(lines[-1] + "\n")
                continue
            if a.exchange:
                plain, pms = timed(rows, B, rack_of, R, size, cap, None)
                res, xms = timed(rows, B, rack_of, R, size, cap, None, exchange=True)
                pm, xm = float(np.median(pms)), float(np.median(xms))
                lb = max(res.lower_bound, 1)
                line = {"workload": name, "sigma": sigma, "brokers": B, "racks": R, "partitions": len(rows), "max_per_rack": cap, "move_leaders": not a.keep_leaders,
                        "max_rounds": a.max_rounds, "lower_bound": res.lower_bound, "peak_before": res.peak_before,
                        "peak_over_bound": [round(plain.peak_after / lb, 7), round(res.peak_after / lb, 7)], "peak_after": [plain.peak_after, res.peak_after],
                        "peak_of_moves": res.peak_of_moves, "bytes_moved": [plain.bytes_moved, res.bytes_moved], "bytes_total": total,
                        "rounds": [int(plain.stats[0]), int(res.stats[0])], "move_rounds": int(res.stats[0] - res.stats[8]), "exchange_rounds": res.exchange_rounds,
                        "exchanges": res.exchanges, "exchange_proposals": res.exchange_proposals, "launches": [int(plain.stats[3]), int(res.stats[3])],
                        "stopped_by_max_rounds": [int(plain.stats[5]), int(res.stats[5])], "wall_ms_median": [round(pm, 3), round(xm, 3)], "wall_ms": [pms, xms],
                        "ms_per_move_round": round(pm / max(int(plain.stats[0]), 1), 4),
                        "ms_per_exchange_round": round((xm - pm) / max(res.exchange_rounds, 1), 4), "changes_nothing": res.exchanges == 0}
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
                if a.write:
                    with open(os.path.join(ROOT, "profiles", "disk_x_time.txt"), "a") as f:
                        f.write(lines[-1] + "\n")
                continue
            for pct in [None] if a.max_bytes_pct is None else a.max_bytes_pct.split(","):   # None: kao_balance_disk
                max_bytes = None if pct is None else 2 ** 64 - 1 if pct == "none" else int(total * float(pct) / 100)
                capacity = None if a.capacity is None else np.where((np.arange(B) % 2 == 0) & (a.capacity == "4:1"), 4, 1).astype(np.int64) * 2 ** 36
                res, ms = timed(rows, B, rack_of, R, size, cap, max_bytes, capacity)
                line = {"workload": name, "sigma": sigma, "brokers": B, "racks": R, "partitions": len(rows), "max_per_rack": cap,
                        "move_leaders": not a.keep_leaders, "status": res.status, "peak_before": res.peak_before, "peak_after": res.peak_after,
                        "lower_bound": res.lower_bound, "peak_over_bound": round(res.peak_after / max(res.lower_bound, 1), 5),
                        "largest_partition": int(size.max()), "replicas_moved": res.n_moved, "bytes_moved": res.bytes_moved, "bytes_total": total,
                        "moved_share": round(res.bytes_moved / max(total, 1), 5)}
                if pct is not None:
                    line.update({"max_bytes_pct": pct, "max_bytes": max_bytes, "bytes_left": max_bytes - res.bytes_moved})
                if capacity is not None:
                    def peak_ppm(S):
                        b = max(range(B), key=lambda i: (int(S[i]) * 10 ** 6 // int(capacity[i]), -i))
                        return int(S[b]) * 10 ** 6 // int(capacity[b])
                    held = rows != 0xFFFF
                    plain = balance_disk_arrays(rows, B, rack_of, R, size, cap, not a.keep_leaders, max_bytes=max_bytes)   # the byte planner's plan
                    S = np.zeros(B, dtype=np.int64)
                    np.add.at(S, plain.rows.astype(np.int64)[held], np.broadcast_to(size[:, None], rows.shape)[held])
                    line.update({"capacity": a.capacity, "peak_before_capacity": res.peak_before_capacity, "peak_after_capacity": res.peak_after_capacity,
                                 "lower_bound_den": res.lower_bound_den, "peak_before_ppm": res.peak_before * 10 ** 6 // res.peak_before_capacity,
                                 "peak_after_ppm": res.peak_after * 10 ** 6 // res.peak_after_capacity,
                                 "lower_bound_ppm": res.lower_bound * 10 ** 6 // res.lower_bound_den, "mean_ppm": total * 10 ** 6 // int(capacity.sum()),
                                 "byte_plan_peak_ppm": peak_ppm(S), "byte_plan_rounds": int(plain.stats[0])})
                    line["peak_over_bound"] = round((res.peak_after * res.lower_bound_den) / max(res.lower_bound * res.peak_after_capacity, 1), 5)
                line.update({k: int(v) for k, v in zip(CAPACITY_STAT_KEYS if capacity is not None else STAT_KEYS if pct is None else BUDGET_STAT_KEYS, res.stats)})
                line["wall_ms_median"] = round(float(np.median(ms)), 3)
                if pct is not None:
                    line["wall_ms"] = ms
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    if a.write and not a.exchange and a.drain is None and a.band is None:
        name = "disk_capacity_time.txt" if a.capacity is not None else "disk_time.txt" if a.max_bytes_pct is None else "disk_budget_time.txt"
        with open(os.path.join(ROOT, "profiles", name), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
