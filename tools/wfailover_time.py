"""Times kao_failover_order_weighted on the instances of tools/failover_time.py (BASELINE config 4 after a drift with its 200 topics
concatenated, 300 brokers x 9,000 partitions, 1000 brokers x 100,000 partitions at RF 3), each in both scopes and with log-normal
weights around 2^20 at sigma 0.7 and 1.5 (tests/wfailover_ref.py lognormal_weights).  One JSON line per case, scope and sigma: the worst
peak before and after, the worst peak_after / lower_bound over the scenarios, the proven scenarios among those with work, the stats
and the wall time of the call (median of --reps after one warm-up, dry_run; it includes the host validation, the upload and the
read-back).  With --ref the restatement of the rounds (tests/wfailover_ref.py descend) is timed on this machine's CPU beside it, its
values are compared, and the ratio is printed.  For kernel times run it under `rocprofv3 --kernel-trace --stats --` (in a run of its
own).  Writes the lines to profiles/wfailover_time.txt with --write."""
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
    ap.add_argument("--cases", default="config4,many,large")
    ap.add_argument("--scopes", default="broker,rack")
    ap.add_argument("--sigmas", default="0.7,1.5")
    ap.add_argument("--ref", action="store_true", help="also time the numpy restatement of each case on the CPU")
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/wfailover_time.txt as well")
    a = ap.parse_args()
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.failover import WEIGHTED_STAT_KEYS, _from_topics, failover_order_weighted_arrays
    import failover_ref as fr
    import wfailover_ref as wf
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
        for sigma in [float(s) for s in a.sigmas.split(",")]:
            weight = wf.lognormal_weights(len(rows), sigma, 5)
            for scope in a.scopes.split(","):
                res = failover_order_weighted_arrays(rows, B, rack_of, R, scope, weight, dry_run=True)   # warm-up
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res = failover_order_weighted_arrays(rows, B, rack_of, R, scope, weight, dry_run=True)
                    ms.append(1e3 * (time.perf_counter() - t0))
                scen = [[int(x) for x in s] for s in res.scen.tolist()]
                work = [s for s in scen if s[0]]
                line = {"workload": name, "scope": scope, "sigma": sigma, "brokers": int(B), "racks": int(R), "partitions": int(rows.shape[0]),
                        "width": int(rows.shape[1]), "scenarios_with_work": len(work), "largest_scenario": max(s[0] for s in scen),
                        "worst_peak_before": max(s[2] for s in scen), "worst_peak_after": max(s[3] for s in scen),
                        "worst_peak_over_bound": round(max([s[3] / s[4] for s in work if s[4]] + [1.0]), 4),
                        "proven_with_work": sum(s[3] == s[4] for s in work), "status": res.status, "offline": sum(s[1] for s in scen),
                        "reordered": res.n_reordered, **{k: int(v) for k, v in zip(WEIGHTED_STAT_KEYS, res.stats)},
                        "wall_ms_median": round(float(np.median(ms)), 3)}
                if a.ref:
                    t0 = time.perf_counter()
                    ref = wf.descend(rows, weight, B, rack_of, 0 if scope == "broker" else 1, R)
                    line["ref_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
                    line["ref_equal"] = bool(ref["scen"] == scen)
                    line["ref_over_gpu"] = round(line["ref_ms"] / line["wall_ms_median"], 1)
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "wfailover_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
