"""Generates tests/golden/cx_large.npz: what oracle/kao_cycle.py computes on the drifted 940-broker, 8-rack, 1200-partition RF-3
topic (n = 949 nodes, row stride 960: the size at which a squaring is ONE launch of the unsplit kernel, as on the 1000-broker
workloads).  A squaring of the oracle takes about 18 s at this size, a round about 3 minutes, so tests/test_gpu_cycle_paths.py
compares the device with this file instead of the live oracle.  "parity unpinned": the project's own oracle, nothing else.

Stored, for the start A0 = port_search(t, 3, 0, 1, 2048):
  start            [P, RF] uint16
  diag             [3 layers, 4 levels, n] int32: the diagonal of every dist matrix of the round on `start`
  bands_dist       [3, 4, nb, 32] uint8: SHA-256 of rows 64*b .. 64*b+63 of each dist matrix as int32 [n, n], C order -- the
  bands_mid        [3, 4, nb, 32]        array kao.cycle_matrices returns; a mismatch names the 64-row band, the blockIdx.y of a
  bands_slot       [3, nb, 32]           squaring (mid as int32, level 0 unused; slot as uint32 = the low word of the edge key)
  l_round, l_start the L layer is priced on the F closure only in a round whose F closure has no negative diagonal entry (the
                   round that also transposes it): index and assignment of the first such round; bands_dist[2], bands_mid[2],
                   bands_slot[2] and diag[2] are taken from it; diag_l_round [3, 4, n] are all its diagonals (l_round = 0: the same round as everything else)
  improved, history the assignment after kc.improve(t, start, 2) and its per-round info as JSON

Run in the build container:  python tests/golden/make_golden_cx_large.py [dump.npz]      (about 10 minutes on one core; the
optional argument keeps the raw matrices of every round, ~100 MB, for looking at a mismatch)
"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import kao_cycle as kc  # noqa: E402
import kao_oracle as ko  # noqa: E402
import kao_port as kp  # noqa: E402
from kafka_assignment_optimizer_amd import synthetic  # noqa: E402

SHAPE = (940, 8, 1200, 3)
MAX_EXTRA_ROUNDS = 3


def oracle_topic(B, R, P, rf, frac=0.2, seed=1):
    pt = synthetic.drift(synthetic.make_cluster(B, R, 1, P, rf, [], []), frac, seed)[0]
    return ko.Topic(name=pt.name, broker_ids=np.array(pt.broker_ids), rack_of=np.array(pt.rack_of), n_racks=pt.n_racks,
                    n_partitions=pt.n_partitions, rf=pt.rf, current=np.array(pt.current), weights=pt.weights)


def bands(M, dtype):
    M = np.ascontiguousarray(np.asarray(M).astype(dtype))
    return np.array([np.frombuffer(hashlib.sha256(M[i:i + 64].tobytes()).digest(), dtype=np.uint8) for i in range(0, M.shape[0], 64)])


def layer_of(rd, layer):
    return ((rd.DF, rd.MF, rd.EF), (rd.DS, rd.MS, rd.ES), (rd.DL, rd.ML, rd.EL))[layer]


def f_has_cycle(rd):
    return any((np.diag(rd.DF[lev])[:rd.B] < 0).any() for lev in range(1, kc.LEVELS + 1))


def main():
    t0 = time.perf_counter()
    kp.build()
    t = oracle_topic(*SHAPE)
    r = kp.port_search(t, 3, 0, 1, 2048)
    assert r["best_obj"] >= 0, "no feasible start"
    start = np.asarray(r["best"]).astype(np.uint16).reshape(t.n_partitions, t.rf)
    print("start objective", r["best_obj"], flush=True)

    rounds = []

    class Recorded(kc.Round):              # keep the Round objects kc.improve builds: each costs three minutes
        def __init__(self, t, A):
            super().__init__(t, A)
            rounds.append(self)
            print("round", len(rounds), "F cycle" if f_has_cycle(self) else "no F cycle", len(self.cycle_candidates()), "cycle candidates",
                  round(time.perf_counter() - t0), "s", flush=True)

    plain_round = kc.Round
    kc.Round = Recorded
    try:
        improved, hist = kc.improve(t, start, 2)
        A = improved
        for _ in range(MAX_EXTRA_ROUNDS):          # only while every round so far had an F cycle
            if not all(f_has_cycle(rd) for rd in rounds):
                break
            A, _ = kc.round_step(t, A)
            if A is None:
                break
    finally:
        kc.Round = plain_round
    l_round = next((i for i, rd in enumerate(rounds) if not f_has_cycle(rd)), -1)
    assert l_round >= 0, "no round without an F cycle: raise MAX_EXTRA_ROUNDS"

    n = rounds[0].n
    nb = (n + 63) // 64
    diag = np.zeros((3, 4, n), dtype=np.int32)
    b_dist = np.zeros((3, 4, nb, 32), dtype=np.uint8)
    b_mid = np.zeros((3, 4, nb, 32), dtype=np.uint8)
    b_slot = np.zeros((3, nb, 32), dtype=np.uint8)
    for layer in range(3):
        Ds, Ms, E = layer_of(rounds[l_round if layer == 2 else 0], layer)
        b_slot[layer] = bands(E & np.uint64(0xFFFFFFFF), np.uint32)
        for lev in range(4):
            diag[layer, lev] = np.diag(Ds[lev])
            b_dist[layer, lev] = bands(Ds[lev], np.int32)
            if lev:
                b_mid[layer, lev] = bands(Ms[lev], np.int32)
    out = dict(shape=np.array(SHAPE, dtype=np.int32), start=start, start_objective=np.int64(r["best_obj"]), diag=diag, bands_dist=b_dist,
               bands_mid=b_mid, bands_slot=b_slot, l_round=np.int32(l_round), l_start=rounds[l_round].A.astype(np.uint16),
               diag_l_round=np.array([[np.diag(layer_of(rounds[l_round], layer)[0][lev]) for lev in range(4)] for layer in range(3)], dtype=np.int32),
               improved=np.asarray(improved).astype(np.uint16), history=np.array(json.dumps(hist)),
               seconds=np.float64(round(time.perf_counter() - t0, 1)))
    np.savez_compressed(os.path.join(HERE, "cx_large.npz"), **out)
    if len(sys.argv) > 1:
        raw = {}
        for i, rd in enumerate(rounds):
            raw[f"A{i}"] = rd.A
            for layer in range(3):
                Ds, Ms, E = layer_of(rd, layer)
                raw[f"E{i}_{layer}"] = E
                for lev in range(4):
                    raw[f"D{i}_{layer}_{lev}"] = Ds[lev].astype(np.int32)
                    if lev:
                        raw[f"M{i}_{layer}_{lev}"] = Ms[lev].astype(np.int32)
        np.savez_compressed(sys.argv[1], **raw)
    print("l_round", l_round, "history", hist, "seconds", out["seconds"], flush=True)


if __name__ == "__main__":
    main()
