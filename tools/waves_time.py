"""Times kao_plan_waves on the large wave-planning families of tests/test_gpu_waves.py: BASELINE config 4 as one cluster-wide
plan (10,000 partitions) and drift100k against a further drift (100,000 partitions), at k = 1, 2, 5.  One JSON line per case:
partitions changed, waves, lower bound and the wall time of the call (median of --reps after one warm-up call; it includes the
host validation, the uploads and the read-back).  For kernel times run it under `rocprofv3 --kernel-trace --stats --`.
--sized times kao_plan_waves_sized instead: sizes from tests/waves_sized_ref.gen_sizes (log-uniform 1 KiB .. 1 TiB, 10 % empty,
seed 7) at the byte caps of --caps (TiB) with the count caps of --ks (0 = none).  Round counts are not visible from the host: count
the k_wave_round launches in the trace (one per round, in batches of 32).
--headroom times kao_plan_waves_headroom on the same sizes and caps, with kao_plan_waves_sized timed beside it as the yardstick:
once at capacity 2^63 everywhere (where wave[] must equal the sized planner's) and once at floor(max(stored, final) * 1.1), stored
and final being the sizes of a broker's current and target rows.  Its rounds are stats[4] of the call."""
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
    ap.add_argument("--headroom", action="store_true")
    ap.add_argument("--caps", default="4,1", help="byte caps in TiB (with --sized and --headroom)")
    a = ap.parse_args()
    if a.headroom:
        return headroom(a)
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


def _median_ms(call, reps):
    import numpy as np
    out = call()   # warm-up
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, round(float(np.median(ms)), 3)


def headroom(a):
    import numpy as np
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.waves import plan_waves_headroom_arrays, plan_waves_sized_arrays
    import waves_ref as wr
    import waves_sized_ref as sr
    kao.init(0)
    for name, make in (("config4", wr.config4_pair), ("drift100k", wr.drift100k_pair)):
        cur, tgt, B = make()
        size = sr.gen_sizes(cur.shape[0], 7)
        held = []
        for rows in (cur, tgt):
            h = np.zeros(B + 1, dtype=np.uint64)
            np.add.at(h, np.where(rows == wr.NONE, B, rows).reshape(-1), np.repeat(size, rows.shape[1]))
            held.append(h[:B])
        stored = held[0]
        tight = np.array([max(int(x), int(y)) * 11 // 10 for x, y in zip(*held)], dtype=np.uint64)
        unlimited = np.full(B, 1 << 63, dtype=np.uint64)
        for cap in (float(x) for x in a.caps.split(",")):
            C = int(cap * (1 << 40))
            for k in (int(x) for x in a.ks.split(",")):
                (sw, snw, slb), sized_ms = _median_ms(lambda: plan_waves_sized_arrays(cur, tgt, B, size, C, k), a.reps)
                row = {"workload": name, "brokers": B, "partitions": int(cur.shape[0]), "C_TiB": cap, "k": k, "sized_n_waves": snw,
                       "lower_bound": slb, "sized_wall_ms_median": sized_ms}
                for tag, capacity in (("unlimited", unlimited), ("x1.1", tight)):
                    (w, nw, lb, st), ms = _median_ms(lambda: plan_waves_headroom_arrays(cur, tgt, B, size, stored, capacity, C, k), a.reps)
                    row[tag] = {"n_waves": nw, "stuck": int(st[0]), "stuck_bytes": int(st[1]), "winning_order": int(st[2]), "orders": int(st[3]),
                                "rounds": int(st[4]), "min_free": int(st[5]), "wall_ms_median": ms}
                    if tag == "unlimited":
                        row[tag]["equals_sized"] = bool((w == sw).all() and nw == snw and lb == slb)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
