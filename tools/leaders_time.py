"""Times kao_balance_leaders on the families of tests/test_gpu_leaders.py: BASELINE config 4 after a drift as one batch of 200
topics (one call per topic, the batch's wall time), the ring instance (60 brokers, 1800 partitions, seed 0) and the large instance
(1000 brokers x 100,000 partitions, RF 3).  One JSON line per case: leader changes, stats[0..3] and stats[6] (phases, relaxation
rounds, augmenting paths, longest path in arcs, kernel launches) and the wall time of the calls (median of --reps after one warm-up;
it includes the host validation, the upload, the read-back and the K-eval objective).  With --highs the HiGHS LP of the same
instance is timed on this machine's CPU beside it and the ratio is printed.  For kernel times run it under
`rocprofv3 --kernel-trace --stats --` (in a run of its own).  Writes the lines to profiles/leaders_time.txt with --write."""
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
    ap.add_argument("--cases", default="config4,ring,large")
    ap.add_argument("--highs", action="store_true", help="also time the HiGHS LP of each instance on the CPU")
    ap.add_argument("--write", action="store_true", help="write the lines to profiles/leaders_time.txt as well")
    a = ap.parse_args()
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd import Topic
    from kafka_assignment_optimizer_amd.leaders import balance_leaders
    import leaders_ref as lr
    kao.init(0)

    def topic(rows, B, lo, hi, n_racks):
        rows = np.asarray(rows, dtype=np.uint16)
        return Topic(name="t", broker_ids=np.arange(B), rack_of=np.arange(B) % n_racks, n_racks=n_racks, n_partitions=rows.shape[0],
                     rf=rows.shape[1], current=rows, bounds_override={"lead_lo": lo, "lead_hi": hi})

    cases = {}
    if "config4" in a.cases:
        cases["config4_200_topics"] = lr.config4_topics()
    if "ring" in a.cases:
        cases["ring_60x1800_seed0"] = [topic(*lr.ring_instance(0, 60, 1800), 2)]
    if "large" in a.cases:
        cases["large_1000x100000"] = [topic(*lr.large_instance(), 10)]
    lines = []
    for name, topics in cases.items():
        res = [balance_leaders(t) for t in topics]   # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = [balance_leaders(t) for t in topics]
            ms.append(1e3 * (time.perf_counter() - t0))
        stats = np.sum([r.stats for r in res], axis=0)
        line = {"workload": name, "topics": len(topics), "brokers": topics[0].n_brokers, "partitions": int(sum(t.n_partitions for t in topics)),
                "status": sorted({r.status for r in res}), "n_changed": int(sum(r.n_changed for r in res)), "phases": int(stats[0]),
                "rounds": int(stats[1]), "paths": int(stats[2]), "longest_path": int(max(r.stats[3] for r in res)), "launches": int(stats[6]),
                "wall_ms_median": round(float(np.median(ms)), 3)}
        if a.highs:
            t0 = time.perf_counter()
            opt = 0
            for t in topics:
                bd = kao.derive_bounds(t)
                opt += lr.lp_optimum(np.asarray(t.current, dtype=np.int64), t.n_brokers, bd["lead_lo"], bd["lead_hi"]) or 0
            line["highs_lp_optimum"] = opt
            line["highs_lp_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            line["highs_over_gpu"] = round(line["highs_lp_ms"] / line["wall_ms_median"], 1)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "leaders_time.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
