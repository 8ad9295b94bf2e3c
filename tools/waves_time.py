"""Times kao_plan_waves on the large wave-planning families of tests/test_gpu_waves.py: BASELINE config 4 as one cluster-wide
plan (10,000 partitions) and drift100k against a further drift (100,000 partitions), at k = 1, 2, 5.  One JSON line per case:
partitions changed, waves, lower bound and the wall time of the call (median of --reps after one warm-up call; it includes the
host validation, the uploads and the read-back).  For kernel times run it under `rocprofv3 --kernel-trace --stats --`."""
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
    ap.add_argument("--ks", default="1,2,5")
    a = ap.parse_args()
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.waves import plan_waves_arrays
    import waves_ref as wr
    kao.init(0)
    for name, make in (("config4", wr.config4_pair), ("drift100k", wr.drift100k_pair)):
        cur, tgt, B = make()
        changed = int((cur != tgt).any(axis=1).sum())
        for k in (int(x) for x in a.ks.split(",")):
            plan_waves_arrays(cur, tgt, B, k)
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                wave, nw, lb = plan_waves_arrays(cur, tgt, B, k)
                ms.append(1e3 * (time.perf_counter() - t0))
            print(json.dumps({"workload": name, "brokers": B, "partitions": int(cur.shape[0]), "changed": changed, "k": k,
                              "n_waves": nw, "lower_bound": lb, "first_fit_degree_order": wr.first_fit_waves(cur, tgt, k),
                              "wall_ms_median": round(float(np.median(ms)), 3)}), flush=True)


if __name__ == "__main__":
    main()
