"""Times kao_failover_order on: BASELINE config 4 after a drift with its 200 topics concatenated over the one broker index, the
300 brokers x 9,000 partitions instance of tests/test_gpu_failover.py, and 1000 brokers x 100,000 partitions at RF 3 (leaders p % B,
followers in other racks), each in both scopes.  One JSON line per case and scope: the worst peak before and after, the swaps,
stats (scenarios, probes, phases, relaxation rounds, paths, longest path, launches, largest scenario) and the wall time of the call
(median of --reps after one warm-up; it includes the host validation, the upload and the read-back).  With --highs the HiGHS
reference of the same scenarios (tests/failover_ref.py scenario_optimum) is timed on this machine's CPU beside it, its values are
compared, and the ratio is printed.  For kernel times run it under `rocprofv3 --kernel-trace --stats --` (in a run of its own).
Writes the lines to profiles/failover_time.txt with --write."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="config4,many,large")
    ap.add_argument("--scopes", default="broker,rack")
    ap.add_argument("--highs", action="store_true", help="also time the HiGHS reference of each case on the CPU")
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/failover_time.txt as well")
    a = ap.parse_args()
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.failover import STAT_KEYS, _from_topics, failover_order_arrays
    import failover_ref as fr
    kao.init(0)

    cases = {}
    if "config4" in a.cases:
        import leaders_ref as lr
        topics = lr.config4_topics()
        fi = _from_topics(topics, None)
        cases["config4_200_topics_concatenated"] = (fi.rows, len(fi.broker_ids), fi.rack_of, topics[0].n_racks)
    if "many" in a.cases:
        cases["many_300x9000"] = fr.many_instance()
    if "large" in a.cases:
        cases["large_1000x100000"] = fr.many_instance(B=1000, R=10, P=100000)
    lines = []
    for name, (rows, B, rack_of, R) in cases.items():
        for scope in a.scopes.split(","):
            res = failover_order_arrays(rows, B, rack_of, R, scope)   # warm-up
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = failover_order_arrays(rows, B, rack_of, R, scope)
                ms.append(1e3 * (time.perf_counter() - t0))
            line = {"workload": name, "scope": scope, "brokers": int(B), "racks": int(R), "partitions": int(rows.shape[0]), "width": int(rows.shape[1]),
                    "worst_peak_before": int(res.scen[:, 2].max()), "worst_peak_after": int(res.scen[:, 3].max()), "offline": int(res.scen[:, 1].sum()),
                    "reordered": res.n_reordered, **{k: int(v) for k, v in zip(STAT_KEYS, res.stats)}, "wall_ms_median": round(float(np.median(ms)), 3)}
            if a.highs:
                t0 = time.perf_counter()
                opt = fr.scenario_optimum(rows, B, rack_of, 0 if scope == "broker" else 1, R)
                line["highs_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                line["highs_equal"] = bool((opt == res.scen).all())
                line["highs_over_gpu"] = round(line["highs_ms"] / line["wall_ms_median"], 1)
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "failover_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
