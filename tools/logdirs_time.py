"""Times kao_balance_logdirs on three shapes of tests/logdirs_ref.py's log-normal family, each with sizes of
sigma 0.7 and 1.5 on a placement skewed 1:4 over a broker's dirs: 1000 brokers x 12 dirs x 300 replicas (the 1000-broker, 100,000-
partition, RF 3 cluster of the other tables), 100 x 24 x 3,000, and one broker x 12 x 2,500.  One JSON line per case: the peak over
all dirs before and after, the worst and the mean peak_after / lower_bound over the brokers, the brokers proven optimal, replicas and
bytes moved, the bytes stored, the stats (rounds summed and of the slowest broker, moves, proposals, kernel launches) and the wall
time of the call with dry_run (median of --reps after one warm-up; it includes the host validation, the upload and the read-back of
the counters and of per_broker, and ends in a stream synchronise).  --ref times the numpy restatement on the single-broker case as
well, on one host core.  For kernel times run it under `rocprofv3 --kernel-trace --stats --` (in a run of its own, --reps 1).
Writes the lines to profiles/logdirs_time.txt with --write."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"cluster": (1000, 12, 300), "dense": (100, 24, 3000), "one": (1, 12, 2500)}   # brokers, dirs a broker, replicas a broker


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="cluster,dense,one")
    ap.add_argument("--sigmas", default="0.7,1.5")
    ap.add_argument("--ref", action="store_true", help="time tests/logdirs_ref.descend on the single-broker case too")
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/logdirs_time.txt as well")
    a = ap.parse_args()
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.logdirs import STAT_KEYS, balance_logdirs_arrays
    import logdirs_ref as lr
    kao.init(0)
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
