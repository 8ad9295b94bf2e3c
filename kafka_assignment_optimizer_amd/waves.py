"""Waves: a reassignment plan split for execution with at most `k` partition movements per broker per wave (kao_plan_waves,
DESIGN.md section 4g).

    kao-cli ... --out plan.json
    python -m kafka_assignment_optimizer_amd.waves --current current.json --plan plan.json --max-per-broker 2 --out-prefix wave

writes wave1.json .. waveN.json, each a reassignment document `kafka-reassign-partitions --execute` takes on its own.  A partition
moves data when the plan adds brokers to it; its participants are the added brokers and its current preferred leader, from which
new followers copy.  Balance bands are not enforced on the states between waves.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from . import _ffi
from .model import NONE
from .solver import _check


@dataclass
class WaveInput:
    """The two documents over one broker index: every broker id of either document (a decommissioned broker stays a source)."""
    keys: List[Tuple[str, int]]   # (topic, partition) in the order of the current document
    broker_ids: np.ndarray        # dense index -> broker id, ascending
    current: np.ndarray           # [P, width] uint16 dense, NONE-padded
    target: np.ndarray            # [P, width] uint16 dense, NONE-padded
    target_replicas: List[List[int]] = field(default_factory=list)   # broker ids, as the plan lists them


@dataclass
class WavePlan:
    n_waves: int
    lower_bound: int
    optimal: bool                 # n_waves == lower_bound
    wave: np.ndarray              # [P] int32 per partition of WaveInput.keys; -1 = unchanged
    waves: List[dict]             # one reassignment document per wave, wave 0 first
    input: WaveInput


def _entries(doc: dict, what: str):
    out = {}
    for e in doc.get("partitions", []):
        key = (str(e["topic"]), int(e["partition"]))
        if key in out:
            raise ValueError(f"{what}: partition {key[0]}-{key[1]} listed twice")
        out[key] = [int(b) for b in e["replicas"]]
    return out


def parse_pair(current_doc: dict, plan_doc: dict) -> WaveInput:
    """Both reassignment documents as rows over the union broker index.  A partition missing from the plan keeps its current
    replicas (unchanged); a partition of the plan that the current document does not have is a ValueError."""
    cur = _entries(current_doc, "current")
    plan = _entries(plan_doc, "plan")
    unknown = [k for k in plan if k not in cur]
    if unknown:
        raise ValueError(f"plan names partitions the current assignment does not have: {unknown[:5]}")
    keys = list(cur)
    tgt = [plan.get(k, cur[k]) for k in keys]
    ids = sorted({b for r in cur.values() for b in r} | {b for r in tgt for b in r})
    dense = {b: i for i, b in enumerate(ids)}
    width = max([1] + [len(r) for r in cur.values()] + [len(r) for r in tgt])
    cur_rows = np.full((len(keys), width), NONE, dtype=np.uint16)
    tgt_rows = np.full((len(keys), width), NONE, dtype=np.uint16)
    for i, k in enumerate(keys):
        for j, b in enumerate(cur[k]):
            cur_rows[i, j] = dense[b]
        for j, b in enumerate(tgt[i]):
            tgt_rows[i, j] = dense[b]
    return WaveInput(keys=keys, broker_ids=np.array(ids, dtype=np.int64), current=cur_rows, target=tgt_rows, target_replicas=tgt)


def plan_waves_arrays(current: np.ndarray, target: np.ndarray, n_brokers: int, max_per_broker: int, seed: int = 1):
    """kao_plan_waves on dense rows ([P, width] each, NONE-padded): (wave int32[P], n_waves, lower_bound)."""
    cur = np.ascontiguousarray(current, dtype=np.uint16)
    tgt = np.ascontiguousarray(target, dtype=np.uint16)
    if cur.shape != tgt.shape or cur.ndim != 2:
        raise ValueError("current and target must be [P, width] arrays of one shape")
    P, W = cur.shape
    wave = np.zeros(max(P, 1), dtype=np.int32)
    nw, lb = C.c_int32(0), C.c_int32(0)
    u16, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_int32)
    _check(_ffi.load().kao_plan_waves(int(n_brokers), int(P), int(W), cur.ctypes.data_as(u16), tgt.ctypes.data_as(u16),
                                      int(max_per_broker), int(seed) & 0xFFFFFFFFFFFFFFFF, wave.ctypes.data_as(i32), C.byref(nw),
                                      C.byref(lb)), "kao_plan_waves")
    return wave[:P], int(nw.value), int(lb.value)


def plan_waves(current_doc: dict, plan_doc: dict, max_per_broker: int, seed: int = 1) -> WavePlan:
    """Split `plan_doc` (relative to `current_doc`) into waves of at most `max_per_broker` movements per broker."""
    wi = parse_pair(current_doc, plan_doc)
    wave, nw, lb = plan_waves_arrays(wi.current, wi.target, len(wi.broker_ids), max_per_broker, seed)
    docs = [{"version": 1, "partitions": []} for _ in range(nw)]
    for i, (t, p) in enumerate(wi.keys):
        if wave[i] >= 0:
            docs[int(wave[i])]["partitions"].append({"topic": t, "partition": p, "replicas": wi.target_replicas[i]})
    return WavePlan(n_waves=nw, lower_bound=lb, optimal=nw == lb, wave=wave, waves=docs, input=wi)


def main(argv=None) -> int:
    """Python twin of cli/kao-waves: same flags, same files, same exit status (0 ok, 1 error, 2 usage)."""
    ap = argparse.ArgumentParser(prog="kao-waves", description="split a reassignment plan into waves capped per broker")
    ap.add_argument("--current", required=True)
    ap.add_argument("--plan", required=True)
    ap.add_argument("--max-per-broker", type=int, required=True)
    ap.add_argument("--out-prefix", required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--report", action="store_true")
    a = ap.parse_args(argv)
    try:
        with open(a.current) as f:
            cur = json.load(f)
        with open(a.plan) as f:
            plan = json.load(f)
        from .solver import init
        init(a.device)
        res = plan_waves(cur, plan, a.max_per_broker, a.seed)
        for w, doc in enumerate(res.waves):
            with open(f"{a.out_prefix}{w + 1}.json", "w") as f:
                f.write(json.dumps(doc) + "\n")
    except Exception as e:  # noqa: BLE001 -- reported, exit status 1
        print(f"kao-waves: {e}", file=sys.stderr)
        return 1
    if a.report:
        sizes = ",".join(str(len(d["partitions"])) for d in res.waves)
        print(f"waves={res.n_waves} lower_bound={res.lower_bound} optimal={'yes' if res.optimal else 'no'} "
              f"partitions_per_wave={sizes}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
