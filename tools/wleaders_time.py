"""Times kao_balance_leaders_weighted on: BASELINE config 4 after a drift with its 200 topics concatenated over the one broker index
(500 brokers x 10,000 partitions) and the large instance of tests/leaders_ref.py (1000 brokers x 100,000 partitions, RF 3), each
with log-normal weights of sigma 0.7 and 1.5.  One JSON line per case: peaks, lower bound, peak_after / lower_bound, leader
changes, the stats (rounds, moves, proposals, kernel launches, path) and the wall time of the call (median of --reps after one
warm-up; it includes the host validation, the upload and the read-back).  --threshold times both kernel paths (kao_wleaders_test_path)
on 300 brokers x P partitions for a ladder of P: where the single workgroup stops paying is the size threshold of DESIGN.md 4k.
--exchange times kao_balance_leaders_weighted_exchange beside kao_balance_leaders_weighted, in one process and on
the same inputs: wleaders_ref.lognormal_case(B, P, 3, sigma, 7) at 12 x 1,200, 100 x 10,000 (sigma 0.7 and 1.5), 500 x 10,000 and
1000 x 100,000, and 12 x 1,200 on each forced kernel path.  Per instance and call: peak / bound, leader changes, the rounds of both
kinds, the exchanges, the launches, the wall time, and for the exchange call the share of it the host spends building PI and the pair
index (kao_wleaders_last_setup_us).  Writes profiles/wleaders_x_time.txt with --write.
For kernel times run it under `rocprofv3 --kernel-trace --stats --` (in a run of its own).  Writes the lines to
profiles/wleaders_time.txt with --write."""
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
    ap.add_argument("--threshold", action="store_true", help="time both kernel paths on a ladder of sizes instead")
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/wleaders_time.txt as well")
    ap.add_argument("--exchange", action="store_true", help="time kao_balance_leaders_weighted_exchange beside kao_balance_leaders_weighted (see the head of this file)")
    a = ap.parse_args()
    if a.exchange and a.threshold:
        ap.error("--exchange and --threshold are two runs")
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd import _ffi
    from kafka_assignment_optimizer_amd.leaders import WEIGHTED_STAT_KEYS, balance_leaders_weighted_arrays
    import leaders_ref as lr
    import wleaders_ref as wr
    kao.init(0)

    def weights(P, sigma, seed):
        rng = np.random.default_rng(seed)
        return np.maximum(1, np.round(np.exp(rng.normal(np.log(2.0 ** 20), sigma, P)))).astype(np.int64)

    def timed(rows, B, weight, exchange=False):
        res = balance_leaders_weighted_arrays(rows, B, weight, dry_run=True, exchange=exchange)   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = balance_leaders_weighted_arrays(rows, B, weight, dry_run=True, exchange=exchange)
            ms.append(1e3 * (time.perf_counter() - t0))
        return res, round(float(np.median(ms)), 3)

    lines = []
    if a.exchange:
        lib = _ffi.load()
        for B, P, sigma, path in ((12, 1200, 0.7, 0), (100, 10000, 0.7, 0), (100, 10000, 1.5, 0), (500, 10000, 0.7, 0), (1000, 100000, 0.7, 0),
                                  (12, 1200, 0.7, 1), (12, 1200, 0.7, 2)):
            rows, weight = wr.lognormal_case(B, P, 3, sigma, 7)
            lib.kao_wleaders_test_path(path)
            plain, plain_ms = timed(rows, B, weight)
            res, ms = timed(rows, B, weight, exchange=True)
            setup_ms = lib.kao_wleaders_last_setup_us() / 1e3
            lib.kao_wleaders_test_path(0)
            line = {"workload": "lognormal", "brokers": B, "partitions": P, "sigma": sigma, "forced_path": path}
            for tag, r, t in (("plain", plain, plain_ms), ("exchange", res, ms)):
                line.update({f"{tag}_peak_over_bound": round(r.peak_after / max(r.lower_bound, 1), 6), f"{tag}_n_changed": r.n_changed,
                             f"{tag}_all_rounds": int(r.stats[0]), f"{tag}_launches": int(r.stats[3]), f"{tag}_wall_ms_median": t})
            line.update({"single_workgroup": int(res.stats[4]), "move_rounds": int(res.stats[0] - res.stats[8]), "exchange_rounds": int(res.stats[8]),
                         "exchanges": int(res.stats[9]), "exchange_proposals": int(res.stats[10]), "pair_index_entries": int(res.stats[11]),
                         "setup_ms_last": round(setup_ms, 3), "setup_share": round(setup_ms / ms, 3)})
            assert res.peak_after <= plain.peak_after
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    elif a.threshold:
        set_path = _ffi.load().kao_wleaders_test_path
        for P in (500, 1000, 2000, 4000, 8000, 16000, 32000, 64000):
            rows, weight = wr.lognormal_case(300, P, 3, 0.7, 5)
            line = {"workload": "threshold", "brokers": 300, "partitions": P}
            for name, path in (("single", 1), ("multi", 2)):
                set_path(path)
                res, ms = timed(rows, 300, weight)
                set_path(0)
                line.update({"rounds": int(res.stats[0]), f"{name}_launches": int(res.stats[3]), f"{name}_wall_ms_median": ms})
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    else:
        cases = {}   # name -> rows, B
        if "config4" in a.cases:
            topics = lr.config4_topics()
            cases["config4"] = (np.concatenate([np.asarray(t.current, dtype=np.int64) for t in topics]), topics[0].n_brokers)
        if "large" in a.cases:
            rows, B, _, _ = lr.large_instance()
            cases["large"] = (rows, B)
        for name, (rows, B) in cases.items():
            for sigma in (0.7, 1.5):
                weight = weights(len(rows), sigma, 11)
                res, ms = timed(rows, B, weight)
                line = {"workload": name, "sigma": sigma, "brokers": B, "partitions": len(rows), "status": res.status,
                        "peak_before": res.peak_before, "peak_after": res.peak_after, "lower_bound": res.lower_bound,
                        "peak_over_bound": round(res.peak_after / max(res.lower_bound, 1), 5), "heaviest_partition": int(weight.max()),
                        "n_changed": res.n_changed}
                line.update({k: int(v) for k, v in zip(WEIGHTED_STAT_KEYS, res.stats)})
                line["wall_ms_median"] = ms
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "wleaders_x_time.txt" if a.exchange else "wleaders_time.txt"), "a" if a.threshold else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
