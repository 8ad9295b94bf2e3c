"""Times kao_plan_waves on the large wave-planning families of tests/test_gpu_waves.py: BASELINE config 4 as one cluster-wide
plan (10,000 partitions) and drift100k against a further drift (100,000 partitions), at k = 1, 2, 5.  One JSON line per case:
partitions changed, waves, lower bound and the wall time of the call (median of --reps after one warm-up call; it includes the
host validation, the uploads and the read-back).  For kernel times run it under `rocprofv3 --kernel-trace --stats --`.
--sized times kao_plan_waves_sized instead: sizes from tests/waves_sized_ref.gen_sizes (log-uniform 1 KiB .. 1 TiB, 10 % empty,
seed 7) at the byte caps of --caps (TiB) with the count caps of --ks (0 = none).  Round counts are not visible from the host: count
the k_wave_round launches in the trace (one per round, in batches of 32)."""
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
    ap.add_argument("--sized", action="store_true")
    ap.add_argument("--caps", default="4,1", help="byte caps in TiB (with --sized)")
    a = ap.parse_args()
    if a.sized:
        return sized(a)
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


def sized(a):
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.waves import plan_waves_sized_arrays
    import waves_ref as wr
    import waves_sized_ref as sr
    kao.init(0)
    for name, make in (("config4", wr.config4_pair), ("drift100k", wr.drift100k_pair)):
        cur, tgt, B = make()
        size = sr.gen_sizes(cur.shape[0], 7)
        changed = int((cur != tgt).any(axis=1).sum())
        for cap in (float(x) for x in a.caps.split(",")):
            C = int(cap * (1 << 40))
            for k in (int(x) for x in a.ks.split(",")):
                plan_waves_sized_arrays(cur, tgt, B, size, C, k)
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    wave, nw, lb = plan_waves_sized_arrays(cur, tgt, B, size, C, k)
                    ms.append(1e3 * (time.perf_counter() - t0))
                print(json.dumps({"workload": name, "brokers": B, "partitions": int(cur.shape[0]), "changed": changed, "C_TiB": cap,
                                  "k": k, "n_waves": nw, "lower_bound": lb,
                                  "first_fit_order0": sr.first_fit_sized_waves(cur, tgt, size, C, k),
                                  "wall_ms_median": round(float(np.median(ms)), 3)}), flush=True)


if __name__ == "__main__":
    main()
