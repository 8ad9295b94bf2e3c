"""Times kao_balance_leaders_weighted on: BASELINE config 4 after a drift with its 200 topics concatenated over the one broker index
(500 brokers x 10,000 partitions) and the large instance of tests/leaders_ref.py (1000 brokers x 100,000 partitions, RF 3), each
with log-normal weights of sigma 0.7 and 1.5.  One JSON line per case: peaks, lower bound, peak_after / lower_bound, leader
changes, the stats (rounds, moves, proposals, kernel launches, path) and the wall time of the call (median of --reps after one
warm-up; it includes the host validation, the upload and the read-back).  --threshold times both kernel paths (kao_wleaders_test_path)
on 300 brokers x P partitions for a ladder of P: where the single workgroup stops paying is the size threshold of DESIGN.md 4k.
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
    a = ap.parse_args()
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

    def timed(rows, B, weight):
        res = balance_leaders_weighted_arrays(rows, B, weight, dry_run=True)   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = balance_leaders_weighted_arrays(rows, B, weight, dry_run=True)
            ms.append(1e3 * (time.perf_counter() - t0))
        return res, round(float(np.median(ms)), 3)

    lines = []
    if a.threshold:
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
        with open(os.path.join(ROOT, "profiles", "wleaders_time.txt"), "a" if a.threshold else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
