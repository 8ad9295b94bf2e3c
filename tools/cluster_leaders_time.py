"""Times kao_balance_leaders_cluster on: BASELINE config 4 after a drift with its 200 topics concatenated over the one broker index
(topic bands [0, 1]), the mid instance of tests/test_gpu_cluster_leaders.py (100 brokers, 20 topics x 150 partitions, bands [0, 3])
and the large instance of tests/leaders_ref.py (1000 brokers x 100,000 partitions, RF 3) split into 100 topics of 1000 partitions
(bands [0, 2]).  One JSON line per case: peak before and after, leader changes, the stats (probes, phases, relaxation rounds,
augmenting paths, longest path in arcs, kernel launches, pair nodes) and the wall time of the call (median of --reps after one
warm-up; it includes the host validation, the pair index, the upload and the read-back).  With --highs CASES the HiGHS LPs of the
same bisection (tests/cluster_leaders_ref.py optimum) are timed on this machine's CPU beside it.  For kernel times run it under
`rocprofv3 --kernel-trace --stats --` (in a run of its own).  Writes the lines to profiles/cluster_leaders_time.txt with --write."""
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
    ap.add_argument("--cases", default="config4,mid,large")
    ap.add_argument("--highs", default="", help="cases whose HiGHS bisection is timed on the CPU as well, CSV")
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/cluster_leaders_time.txt as well")
    a = ap.parse_args()
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.leaders import CLUSTER_STAT_KEYS, balance_leaders_cluster_arrays
    import cluster_leaders_ref as cr
    import leaders_ref as lr
    kao.init(0)

    cases = {}   # name -> rows, topic_of, B, topic_lo, topic_hi
    if "config4" in a.cases:
        topics = lr.config4_topics()
        rows = np.concatenate([np.asarray(t.current, dtype=np.int64) for t in topics])
        topic_of = np.repeat(np.arange(len(topics)), [t.n_partitions for t in topics])
        cases["config4"] = (rows, topic_of, topics[0].n_brokers, np.zeros(len(topics), dtype=np.int64), np.ones(len(topics), dtype=np.int64))
    if "mid" in a.cases:
        rows, topic_of = cr.mid_case(100, 20, 150, 3, 0)
        cases["mid"] = (rows, topic_of, 100, np.zeros(20, dtype=np.int64), np.full(20, 3))
    if "large" in a.cases:
        rows, B, _, _ = lr.large_instance()
        cases["large"] = (rows, np.arange(len(rows)) // 1000, B, np.zeros(100, dtype=np.int64), np.full(100, 2))
    lines = []
    for name, (rows, topic_of, B, tlo, thi) in cases.items():
        res = balance_leaders_cluster_arrays(rows, B, topic_of, tlo, thi, dry_run=True)   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = balance_leaders_cluster_arrays(rows, B, topic_of, tlo, thi, dry_run=True)
            ms.append(1e3 * (time.perf_counter() - t0))
        line = {"workload": name, "topics": len(tlo), "brokers": B, "partitions": len(rows), "status": res.status,
                "peak_before": res.peak_before, "peak_after": res.peak_after, "n_changed": res.n_changed}
        line.update({k: int(v) for k, v in zip(CLUSTER_STAT_KEYS, res.stats)})
        line["wall_ms_median"] = round(float(np.median(ms)), 3)
        if name in a.highs.split(","):
            t0 = time.perf_counter()
            opt = cr.optimum(rows, topic_of, B, 0, tlo, thi)
            line["highs_optimum"] = opt
            line["highs_bisection_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            line["highs_over_gpu"] = round(line["highs_bisection_ms"] / line["wall_ms_median"], 1)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "cluster_leaders_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
