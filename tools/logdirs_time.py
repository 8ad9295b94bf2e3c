"""Times kao_balance_logdirs on three shapes of tests/logdirs_ref.py's log-normal family, each with sizes of
sigma 0.7 and 1.5 on a placement skewed 1:4 over a broker's dirs: 1000 brokers x 12 dirs x 300 replicas (the 1000-broker, 100,000-
partition, RF 3 cluster of the other tables), 100 x 24 x 3,000, and one broker x 12 x 2,500.  One JSON line per case: the peak over
all dirs before and after, the worst and the mean peak_after / lower_bound over the brokers, the brokers proven optimal, replicas and
bytes moved, the bytes stored, the stats (rounds summed and of the slowest broker, moves, proposals, kernel launches) and the wall
time of the call with dry_run (median of --reps after one warm-up; it includes the host validation, the upload and the read-back of
the counters and of per_broker, and ends in a stream synchronise).  --ref times the numpy restatement on the single-broker case as
well, on one host core.  For kernel times run it under `rocprofv3 --kernel-trace --stats --` (in a run of its own, --reps 1).
Writes the lines to profiles/logdirs_time.txt with --write.

--place times kao_place_logdirs instead, on the same family with a third of each broker's replicas homeless:
1000 x 12 x (200 residents + 100 homeless), 100 x 24 x (2,000 + 1,000) and one broker x 12 x (0 + 2,500), each at both sigmas and
both values of move_residents.  Per line the peak before and after, the peak that Kafka's own rule gives on the same arrivals (each,
in array order, to the dir with the fewest partitions, ties to the lowest index; computed here on the host), peak / bound worst and
mean, the brokers proven, the rounds and the wall time as above; beside it the wall time of kao_balance_logdirs on the same brokers
with the arrivals already resident where Kafka's rule put them, and with --ref that of the numpy restatement (tests/place_ref.py) on
one host core.  The last lines time the single broker with its 2,500 replicas resident and nothing to place: the difference to the
line with 2,500 homeless replicas is what compaction, sort and the greedy pass cost.  Writes profiles/place_time.txt with --write.

--capacity equal|4:1 times kao_balance_logdirs_capacity and kao_place_logdirs_capacity on the shapes of both
tables: every dir 16 GiB (equal), or every fourth dir of a broker a quarter of that (4:1).  Per line the peak utilisation before and
after in parts per million, the utilisation that the BYTE planner's plan reaches on the same input and capacities (its dirs read
back and measured here on the host), rounds, moves, proposals and the wall time as above; beside it, from the same session, the wall
time of the byte sibling on the same input.  With equal capacities the two calls give the same plan, and the difference in time is
what the 128-bit compares and the walk cost.  Writes profiles/logdirs_capacity_time.txt with --write.

--exchange times kao_balance_logdirs_exchange beside kao_balance_logdirs, from the same session and on the
shapes of the first table: per line, for each of the two calls, the peak after, peak / bound worst and mean, the brokers proven,
replicas and bytes moved, the rounds and the wall time as above; for the exchange call the rounds of both kinds, the exchanges, the
exchange proposals and the brokers that end with a lower peak.  Writes profiles/logdirs_x_time.txt with --write."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"cluster": (1000, 12, 300), "dense": (100, 24, 3000), "one": (1, 12, 2500)}   # brokers, dirs a broker, replicas a broker
HOMELESS = {"cluster": 100, "dense": 1000, "one": 2500}                                 # --place: of those, homeless


def kafka_rule(np, B, n, broker, local, home):
    """[R] the dir inside its broker that Kafka gives every homeless replica: in array order, the dir with the fewest partitions."""
    counts = np.zeros((B, n), dtype=np.int64)
    np.add.at(counts, (broker[~home], local[~home]), 1)
    out = local.copy()
    idx = np.nonzero(home)[0]
    order = idx[np.argsort(broker[idx], kind="stable")]            # by broker, array order inside
    per = np.bincount(broker[idx], minlength=B)
    start = np.concatenate([[0], np.cumsum(per)])
    for j in range(int(per.max(initial=0))):                        # the j-th arrival of every broker that has one
        bs = np.nonzero(per > j)[0]
        r = order[start[bs] + j]
        c = np.argmin(counts[bs], axis=1)
        counts[bs, c] += 1
        out[r] = c
    return out


def time_place(a, np, lr):
    import place_ref as pr
    from kafka_assignment_optimizer_amd.logdirs import PLACE_STAT_KEYS, balance_logdirs_arrays, place_logdirs_arrays

    def timed(fn):
        fn()   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = fn()
            ms.append(round(1e3 * (time.perf_counter() - t0), 3))
        return res, ms

    lines = []
    cases = [(name, HOMELESS[name]) for name in a.cases.split(",")] + ([("one", 0)] if "one" in a.cases.split(",") else [])
    for name, h in cases:
        B, n, k = SHAPES[name]
        for sigma in (float(s) for s in a.sigmas.split(",")):
            c = lr.lognormal_case(B, n, k, sigma, 11, zeros=0.0)
            broker, local = c["dir"] // n, c["dir"] % n
            rank = np.empty(len(broker), dtype=np.int64)           # the place of a replica among its broker's, in array order
            order = np.argsort(broker, kind="stable")
            rank[order] = np.arange(len(broker)) - np.repeat(np.arange(B) * k, k)
            home = rank >= k - h
            d = np.where(home, -1, c["dir"])
            kafka = kafka_rule(np, B, n, broker, local, home) + n * broker
            kafka_peak = int(lr.loads(c["dir_start"], kafka, c["size"], c["base"]).max())
            _, bal_ms = timed(lambda: balance_logdirs_arrays(c["dir_start"], kafka, c["size"], c["base"], dry_run=True))
            for move in (False, True):
                args = (c["dir_start"], broker, d, c["size"], c["base"], move)
                res, ms = timed(lambda: place_logdirs_arrays(*args, dry_run=True))
                per = res.per_broker.astype(np.float64)
                ratio = per[:, 1] / np.maximum(per[:, 2], 1)
                line = {"workload": name, "sigma": sigma, "brokers": B, "dirs_per_broker": n, "residents_per_broker": k - h, "homeless_per_broker": h,
                        "move_residents": move, "status": res.status, "peak_before": res.peak_before, "peak_after": res.peak_after, "peak_kafka_rule": kafka_peak,
                        "peak_over_bound_worst": round(float(ratio.max()), 5), "peak_over_bound_mean": round(float(ratio.mean()), 5),
                        "largest_replica": int(c["size"].max()), "replicas_placed": res.n_placed, "bytes_placed": res.bytes_placed, "replicas_moved": res.n_moved,
                        "bytes_moved": res.bytes_moved}
                line.update({key: int(v) for key, v in zip(PLACE_STAT_KEYS, res.stats)})
                line["wall_ms"] = ms
                line["wall_ms_median"] = round(float(np.median(ms)), 3)
                line["balance_after_kafka_rule_wall_ms_median"] = round(float(np.median(bal_ms)), 3)
                if a.ref:
                    t0 = time.perf_counter()
                    ref = pr.place(*args)
                    line["restatement_one_core_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                    assert ref["dir"].tobytes() == place_logdirs_arrays(*args).dir.astype(np.int64).tobytes()
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "place_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def time_capacity(a, np, lr):
    from kafka_assignment_optimizer_amd.logdirs import PLACE_STAT_KEYS, STAT_KEYS, balance_logdirs_arrays, place_logdirs_arrays

    def timed(fn):
        fn()   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = fn()
            ms.append(round(1e3 * (time.perf_counter() - t0), 3))
        return res, ms

    def ppm(L, cap):   # the peak utilisation of the loads L, in parts per million (integer division, as the reports print it)
        at = max(range(len(L)), key=lambda d: (int(L[d]) * 10 ** 6 // int(cap[d]), -d))
        return int(L[at]) * 10 ** 6 // int(cap[at])

    lines = []
    for name in a.cases.split(","):
        B, n, k = SHAPES[name]
        cap = np.full(B * n, 1 << 34, dtype=np.uint64)
        if a.capacity == "4:1":
            cap[np.arange(B * n) % n % 4 == 0] = 1 << 32
        for sigma in (float(s) for s in a.sigmas.split(",")):
            c = lr.lognormal_case(B, n, k, sigma, 11, zeros=0.0)
            forms = [("balance", None)]
            if a.place:
                broker = c["dir"] // n
                rank = np.empty(len(broker), dtype=np.int64)
                rank[np.argsort(broker, kind="stable")] = np.arange(len(broker)) - np.repeat(np.arange(B) * k, k)
                d = np.where(rank >= k - HOMELESS[name], -1, c["dir"])
                forms = [("place", False), ("place", True)]
            for form, move in forms:
                if form == "balance":
                    call = lambda **kw: balance_logdirs_arrays(c["dir_start"], c["dir"], c["size"], c["base"], **kw)
                else:
                    call = lambda **kw: place_logdirs_arrays(c["dir_start"], broker, d, c["size"], c["base"], move, **kw)
                res, ms = timed(lambda: call(dry_run=True, capacity=cap))
                _, byte_ms = timed(lambda: call(dry_run=True))
                L_byte = lr.loads(c["dir_start"], call().dir, c["size"], c["base"])
                L_cap = lr.loads(c["dir_start"], call(capacity=cap).dir, c["size"], c["base"])
                assert ppm(L_cap, cap) == res.peak_after * 10 ** 6 // res.peak_after_frac[1]
                proofs = np.bincount(res.per_broker[:, -1].astype(np.int64), minlength=3)
                line = {"workload": name, "call": form, "capacity": a.capacity, "sigma": sigma, "brokers": B, "dirs_per_broker": n, "replicas_per_broker": k,
                        "status": res.status, "peak_before_ppm": res.peak_before * 10 ** 6 // res.peak_before_frac[1], "peak_after_ppm": ppm(L_cap, cap),
                        "byte_plan_peak_ppm": ppm(L_byte, cap), "replicas_moved": res.n_moved, "bytes_moved": res.bytes_moved,
                        "proof_gap_bound_test": [int(x) for x in proofs[:3]]}
                if form == "place":
                    line.update({"homeless_per_broker": HOMELESS[name], "move_residents": move, "replicas_placed": res.n_placed})
                line.update({key: int(v) for key, v in zip(PLACE_STAT_KEYS if form == "place" else STAT_KEYS, res.stats)})
                line.update({"wall_ms": ms, "wall_ms_median": round(float(np.median(ms)), 3), "byte_sibling_wall_ms": byte_ms,
                             "byte_sibling_wall_ms_median": round(float(np.median(byte_ms)), 3)})
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "logdirs_capacity_time.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")


def time_exchange(a, np, lr):
    from kafka_assignment_optimizer_amd.logdirs import X_STAT_KEYS, balance_logdirs_arrays

    def timed(fn):
        fn()   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = fn()
            ms.append(round(1e3 * (time.perf_counter() - t0), 3))
        return res, ms

    lines = []
    for name in a.cases.split(","):
        B, n, k = SHAPES[name]
        for sigma in (float(s) for s in a.sigmas.split(",")):
            c = lr.lognormal_case(B, n, k, sigma, 11, zeros=0.0)
            args = (c["dir_start"], c["dir"], c["size"], c["base"])
            plain, plain_ms = timed(lambda: balance_logdirs_arrays(*args, dry_run=True))
            res, ms = timed(lambda: balance_logdirs_arrays(*args, dry_run=True, exchange=True))
            assert (res.per_broker[:, 1] <= plain.per_broker[:, 1]).all()
            line = {"workload": name, "sigma": sigma, "brokers": B, "dirs_per_broker": n, "replicas_per_broker": k}
            for tag, r in (("plain", plain), ("exchange", res)):
                per = r.per_broker.astype(np.float64)
                ratio = per[:, 1] / np.maximum(per[:, 2], 1)
                line.update({f"{tag}_status": r.status, f"{tag}_peak_after": r.peak_after, f"{tag}_peak_over_bound_worst": round(float(ratio.max()), 6),
                             f"{tag}_peak_over_bound_mean": round(float(ratio.mean()), 6), f"{tag}_proven": int(r.stats[6]), f"{tag}_replicas_moved": r.n_moved,
                             f"{tag}_bytes_moved": r.bytes_moved, f"{tag}_rounds": int(r.stats[1]), f"{tag}_max_rounds_of_a_broker": int(r.stats[7])})
            line.update({key: int(v) for key, v in zip(X_STAT_KEYS, res.stats)})
            line.update({"brokers_with_a_lower_peak": int((res.per_broker[:, 1] < plain.per_broker[:, 1]).sum()), "plain_wall_ms": plain_ms,
                         "plain_wall_ms_median": round(float(np.median(plain_ms)), 3), "wall_ms": ms, "wall_ms_median": round(float(np.median(ms)), 3)})
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "logdirs_x_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="cluster,dense,one")
    ap.add_argument("--sigmas", default="0.7,1.5")
    ap.add_argument("--ref", action="store_true", help="time tests/logdirs_ref.descend on the single-broker case too")
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/logdirs_time.txt (profiles/place_time.txt with --place) as well")
    ap.add_argument("--place", action="store_true", help="time kao_place_logdirs instead (see the head of this file)")
    ap.add_argument("--capacity", choices=("equal", "4:1"), default=None, help="time the capacity calls (with --place: kao_place_logdirs_capacity); "
                    "--write appends to profiles/logdirs_capacity_time.txt")
    ap.add_argument("--exchange", action="store_true", help="time kao_balance_logdirs_exchange beside kao_balance_logdirs (see the head of this file)")
    a = ap.parse_args()
    if a.exchange and (a.place or a.capacity):
        ap.error("--exchange times the plain balance alone: not with --place or --capacity")
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.logdirs import STAT_KEYS, balance_logdirs_arrays
    import logdirs_ref as lr
    kao.init(0)
    if a.exchange:
        return time_exchange(a, np, lr)
    if a.capacity:
        return time_capacity(a, np, lr)
    if a.place:
        return time_place(a, np, lr)
    lines = []
    for name in a.cases.split(","):
        B, n, k = SHAPES[name]
        for sigma in (float(s) for s in a.sigmas.split(",")):
            c = lr.lognormal_case(B, n, k, sigma, 11, zeros=0.0)
            args = (c["dir_start"], c["dir"], c["size"], c["base"])
            res = balance_logdirs_arrays(*args, dry_run=True)   # warm-up
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = balance_logdirs_arrays(*args, dry_run=True)
                ms.append(round(1e3 * (time.perf_counter() - t0), 3))
            per = res.per_broker.astype(np.float64)
            ratio = per[:, 1] / np.maximum(per[:, 2], 1)
            total = int(c["size"].sum()) + int(c["base"].sum())
            line = {"workload": name, "sigma": sigma, "brokers": B, "dirs_per_broker": n, "replicas_per_broker": k, "status": res.status,
                    "peak_before": res.peak_before, "peak_after": res.peak_after, "peak_over_bound_worst": round(float(ratio.max()), 5),
                    "peak_over_bound_mean": round(float(ratio.mean()), 5), "largest_replica": int(c["size"].max()), "replicas_moved": res.n_moved,
                    "bytes_moved": res.bytes_moved, "bytes_total": total, "moved_share": round(res.bytes_moved / max(total, 1), 5)}
            line.update({key: int(v) for key, v in zip(STAT_KEYS, res.stats)})
            line["wall_ms"] = ms
            line["wall_ms_median"] = round(float(np.median(ms)), 3)
            if a.ref and B == 1:
                t0 = time.perf_counter()
                ref = lr.descend(*args)
                line["restatement_one_core_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                assert ref["dir"].tobytes() == balance_logdirs_arrays(*args).dir.astype(np.int64).tobytes()
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "logdirs_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
