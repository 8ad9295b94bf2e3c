"""Waves: a reassignment plan split for execution with at most `k` partition movements per broker per wave (kao_plan_waves,
DESIGN.md section 4g).

    kao-cli ... --out plan.json
    python -m kafka_assignment_optimizer_amd.waves --current current.json --plan plan.json --max-per-broker 2 --out-prefix wave

writes wave1.json .. waveN.json, each a reassignment document `kafka-reassign-partitions --execute` takes on its own.  A partition
moves data when the plan adds brokers to it; its participants are the added brokers and its current preferred leader, from which
new followers copy.  Balance bands are not enforced on the states between waves.

With partition sizes (`--sizes`, the output of `kafka-log-dirs --describe` or {"partitions": [{"topic", "partition", "size"}]})
and `--max-bytes-per-broker C`, each wave also moves at most C bytes per broker (kao_plan_waves_sized): an added broker receives
size[p], the source sends size[p] once per added broker.  `--max-per-broker` is then optional.

With `--headroom` (implied by `--capacities`, `--default-capacity`, `--max-utilisation PCT`) no wave fills a broker beyond its
capacity, counting what it holds plus everything arriving in the wave (kao_plan_waves_headroom); both caps
are then optional.  Partitions that fit no wave go to PREFIX-stuck.json and the exit status is 3.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

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
    size: Optional[np.ndarray] = None                            # [P] uint64 bytes (sized plans)
    max_broker_bytes: List[int] = field(default_factory=list)    # per wave: the largest bytes one broker moves in it (sized plans)
    bytes_lower_bound: int = 0    # max_b ceil(sum_p min(t_p(b), C) / C) (sized plans with a byte cap)
    # headroom plans (capacity=..): wave[p] = -2 marks a stuck partition
    headroom: bool = False
    stuck: List[Tuple[str, int, List[int]]] = field(default_factory=list)   # (topic, partition, target replicas) of the stuck partitions
    stuck_bytes: int = 0
    stuck_document: Optional[dict] = None                         # the stuck partitions as a reassignment document
    min_free: int = -1            # least free bytes under the effective capacity over (wave, receiving broker); -1: nothing arrives
    min_free_wave: int = -1
    min_free_broker: int = -1     # a broker id
    peak_utilisation_ppm: List[int] = field(default_factory=list)   # per wave: the highest (occ + arr) / capacity over receiving brokers
    stats: Optional[np.ndarray] = None                            # int64[8], see HEADROOM_STAT_KEYS / include/kao.h


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


HEADROOM_STAT_KEYS = ("stuck", "stuck_bytes", "winning_order", "orders", "round_launches", "min_free", "min_free_wave",
                      "min_free_broker")


def _call(name: str, current, target, n_brokers: int, caps, seed: int, size=None, per_broker=None, trailing=()):
    """One library call on dense rows: (wave int32[P], n_waves, lower_bound).  The three calls take the rows, then size[P] and the
    per-broker arrays (stored, capacity) where they have them, then `caps`, the seed, the outputs and what `trailing` holds."""
    cur = np.ascontiguousarray(current, dtype=np.uint16)
    tgt = np.ascontiguousarray(target, dtype=np.uint16)
    if cur.shape != tgt.shape or cur.ndim != 2:
        raise ValueError("current and target must be [P, width] arrays of one shape")
    P, W = cur.shape
    u16, u64, i32 = C.POINTER(C.c_uint16), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    args = [int(n_brokers), int(P), int(W), cur.ctypes.data_as(u16), tgt.ctypes.data_as(u16)]
    arrays = []   # kept alive over the call
    if size is not None:
        sz = np.ascontiguousarray(size, dtype=np.uint64)
        if sz.shape != (P,):
            raise ValueError(f"size must hold one value per partition ({P}), got shape {sz.shape}")
        arrays.append(sz if P else np.zeros(1, dtype=np.uint64))
    if per_broker is not None:
        sto, cap = (np.ascontiguousarray(a, dtype=np.uint64) for a in per_broker)
        if sto.shape != (int(n_brokers),) or cap.shape != (int(n_brokers),):
            raise ValueError(f"stored and capacity must hold one value per broker ({n_brokers}), got shapes {sto.shape} and {cap.shape}")
        arrays += [sto, cap]
    wave = np.zeros(max(P, 1), dtype=np.int32)
    nw, lb = C.c_int32(0), C.c_int32(0)
    args += [a.ctypes.data_as(u64) for a in arrays] + [int(c) for c in caps]
    args += [int(seed) & 0xFFFFFFFFFFFFFFFF, wave.ctypes.data_as(i32), C.byref(nw), C.byref(lb), *trailing]
    _check(getattr(_ffi.load(), name)(*args), name)
    return wave[:P], int(nw.value), int(lb.value)


def plan_waves_arrays(current: np.ndarray, target: np.ndarray, n_brokers: int, max_per_broker: int, seed: int = 1):
    """kao_plan_waves on dense rows ([P, width] each, NONE-padded): (wave int32[P], n_waves, lower_bound)."""
    return _call("kao_plan_waves", current, target, n_brokers, (max_per_broker,), seed)


def plan_waves_sized_arrays(current: np.ndarray, target: np.ndarray, n_brokers: int, size, max_bytes_per_broker: int,
                            max_per_broker: int = 0, seed: int = 1):
    """kao_plan_waves_sized on dense rows: size = bytes per partition ([P]), max_bytes_per_broker = C (0: no byte cap),
    max_per_broker = k (0: no count cap).  (wave int32[P], n_waves, lower_bound)."""
    return _call("kao_plan_waves_sized", current, target, n_brokers, (max_bytes_per_broker, max_per_broker), seed, size=size)


def plan_waves_headroom_arrays(current: np.ndarray, target: np.ndarray, n_brokers: int, size, stored, capacity,
                               max_bytes_per_broker: int = 0, max_per_broker: int = 0, seed: int = 1, with_stats: bool = True):
    """kao_plan_waves_headroom on dense rows: stored / capacity = bytes each broker holds now / may hold ([n_brokers]); both caps may
    be 0.  (wave int32[P] with -2 = stuck, n_waves, lower_bound, stats int64[8] or None when `with_stats` is false)."""
    stats = np.zeros(8, dtype=np.int64) if with_stats else None
    return _call("kao_plan_waves_headroom", current, target, n_brokers, (max_bytes_per_broker, max_per_broker), seed, size=size,
                 per_broker=(stored, capacity), trailing=(stats.ctypes.data_as(C.POINTER(C.c_int64)) if with_stats else None,)) + (stats,)


MAX_SIZE = 1 << 53   # sizes above it are not exact as JSON doubles (the C++ reader): rejected, never rounded


def _size_value(v, what):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= MAX_SIZE:
        raise ValueError(f"{what}: size must be an integer 0..2^53, got {v!r}")
    return v


def parse_sizes(doc_or_text) -> Dict[Tuple[str, int], int]:
    """Partition sizes in bytes, {(topic, partition): size}, from either
      * the output of `kafka-log-dirs --describe` (text: the lines before the JSON line are skipped; or the parsed JSON):
        {"version":1,"brokers":[{"broker":N,"logDirs":[{"partitions":[{"partition":"topic-3","size":123,"isFuture":false}]}]}]}.
        The partition name splits at its last '-'; a partition's size is the largest size of its non-future replicas;
      * a plain document {"partitions":[{"topic":"t","partition":3,"size":123}]}.
    Sizes are integers 0..2^53."""
    doc = doc_or_text
    if isinstance(doc_or_text, (str, bytes)):
        text = doc_or_text.decode() if isinstance(doc_or_text, bytes) else doc_or_text
        try:
            doc = json.loads(text)
        except ValueError:
            doc = None
            for line in text.splitlines():
                if line.lstrip().startswith("{"):
                    doc = json.loads(line)
                    break
            if doc is None:
                raise ValueError("sizes: no JSON document found") from None
    if not isinstance(doc, dict):
        raise ValueError("sizes: expected a JSON object")
    out: Dict[Tuple[str, int], int] = {}
    if "brokers" in doc:
        for br in doc["brokers"]:
            for ld in br.get("logDirs", []):
                for e in ld.get("partitions", []):
                    if e.get("isFuture", False):
                        continue
                    name = str(e["partition"])
                    topic, dash, idx = name.rpartition("-")
                    if not dash or not topic or not idx.isdigit():
                        raise ValueError(f"sizes: partition name {name!r} is not <topic>-<partition>")
                    key = (topic, int(idx))
                    out[key] = max(out.get(key, 0), _size_value(e["size"], name))
    elif "partitions" in doc:
        for e in doc["partitions"]:
            key = (str(e["topic"]), int(e["partition"]))
            if key in out:
                raise ValueError(f"sizes: partition {key[0]}-{key[1]} listed twice")
            out[key] = _size_value(e["size"], f"{key[0]}-{key[1]}")
    else:
        raise ValueError('sizes: expected a "brokers" (kafka-log-dirs) or "partitions" document')
    return out


def traffic(current_row, target_row):
    """Participants of one partition and their traffic in units of its size: [(dense broker, copies)] -- 1 at each added broker,
    n_added at the source current[0]; [] when the partition moves no data."""
    cs = {int(b) for b in current_row if b != NONE}
    add = [int(b) for b in target_row if b != NONE and int(b) not in cs]
    if not add:
        return []
    return [(b, 1) for b in add] + ([(int(current_row[0]), len(add))] if current_row[0] != NONE else [])


def sizes_for(wi: WaveInput, sizes: Dict[Tuple[str, int], int], default_size: Optional[int] = None) -> np.ndarray:
    """size[p] over wi.keys.  A partition that moves data and has no size takes `default_size`; without one it is a ValueError
    naming the first few such partitions.  Partitions that move no data take their size or 0."""
    size = np.zeros(len(wi.keys), dtype=np.uint64)
    missing = []
    for i, key in enumerate(wi.keys):
        if key in sizes:
            size[i] = sizes[key]
        elif traffic(wi.current[i], wi.target[i]):
            if default_size is None:
                missing.append(f"{key[0]}-{key[1]}")
            else:
                size[i] = default_size
    if missing:
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError(f"no size for moving partitions {', '.join(missing[:5])}{more} (give them in --sizes or set --default-size)")
    return size


def wave_bytes(wi: WaveInput, size: np.ndarray, wave: np.ndarray, n_waves: int, max_bytes_per_broker: int = 0):
    """(per wave: the largest bytes one broker moves in it, max_b ceil(sum_p min(t_p(b), C) / C) or 0 when C = 0)."""
    load: Dict[Tuple[int, int], int] = {}
    clamp: Dict[int, int] = {}
    for i in range(len(wi.keys)):
        for b, n in traffic(wi.current[i], wi.target[i]):
            t = n * int(size[i])
            if wave[i] >= 0:   # a stuck partition (headroom plans, wave -2) is in no wave
                load[(int(wave[i]), b)] = load.get((int(wave[i]), b), 0) + t
            if max_bytes_per_broker:
                clamp[b] = clamp.get(b, 0) + min(t, max_bytes_per_broker)
    peak = [0] * n_waves
    for (w, _), v in load.items():
        peak[w] = max(peak[w], v)
    blb = max([-(-v // max_bytes_per_broker) for v in clamp.values()], default=0)
    return peak, blb


def _ppm(num: int, den: int) -> int:
    return int(num) * 10 ** 6 // int(den)


def _log_dirs_table(sizes):
    """The parse_log_dirs table when `sizes` is a kafka-log-dirs document (text, parsed JSON, or such a table), else None."""
    from .logdirs import LogDir, parse_log_dirs
    if isinstance(sizes, dict):
        if sizes and all(isinstance(v, dict) and all(isinstance(d, LogDir) for d in v.values()) for v in sizes.values()):
            return sizes
        return parse_log_dirs(sizes) if "brokers" in sizes else None
    if isinstance(sizes, (str, bytes)):
        text = sizes.decode() if isinstance(sizes, bytes) else sizes
        return parse_log_dirs(text) if '"brokers"' in text else None
    return None


def stored_for(wi: WaveInput, size: np.ndarray, log_dirs=None) -> np.ndarray:
    """stored[b] over wi.broker_ids, the bytes each broker holds now: the sum of size[p] over the current rows that hold b and,
    with a kafka-log-dirs document (or its parse_log_dirs table), the sum of all its entries on b when that is larger -- future
    replicas included, they are bytes on disk.  size[p] being the largest replica, stored[b] then always covers what leaves b."""
    stored = [0] * len(wi.broker_ids)
    for i in range(len(wi.keys)):
        for b in wi.current[i]:
            if b != NONE:
                stored[int(b)] += int(size[i])
    table = None if log_dirs is None else _log_dirs_table(log_dirs)
    if table:
        for j, b in enumerate(wi.broker_ids):
            on_disk = sum(e[2] for d in table.get(int(b), {}).values() for e in d.entries)
            stored[j] = max(stored[j], on_disk)
    return np.array(stored, dtype=np.uint64)


def capacity_for(wi: WaveInput, capacity: Optional[dict] = None, log_dirs=None, default_capacity: Optional[int] = None,
                 max_utilisation: int = 100):
    """(capacity[b], effective capacity[b]) over wi.broker_ids.  A broker's capacity is its entry of `capacity` ({broker id: bytes or
    a string with K/M/G/T}, as disk.capacity_of takes it), else the sum of its log dirs' totalBytes when the kafka-log-dirs
    document reports one for every dir of it (Kafka >= 3.3), else `default_capacity`; a broker with none is a ValueError.  The
    effective capacity is capacity * max_utilisation // 100."""
    from .disk import capacity_of
    if isinstance(max_utilisation, bool) or not isinstance(max_utilisation, (int, np.integer)) or not 1 <= int(max_utilisation) <= 100:
        raise ValueError(f"max_utilisation must be an integer 1..100, got {max_utilisation!r}")
    ids = [int(b) for b in wi.broker_ids]
    named = {int(k): v for k, v in (capacity or {}).items()}
    given = capacity_of([b for b in ids if b in named], named)
    table = dict(zip([b for b in ids if b in named], (int(v) for v in given)))
    dirs = (None if log_dirs is None else _log_dirs_table(log_dirs)) or {}
    out, missing = [], []
    for b in ids:
        totals = [d.total_bytes for d in dirs.get(b, {}).values()]
        if b in table:
            out.append(table[b])
        elif totals and all(t is not None for t in totals) and sum(totals) > 0:
            out.append(sum(totals))
        elif default_capacity is not None:
            out.append(int(default_capacity))
        else:
            missing.append(b)
    if missing:
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError("no capacity for brokers " + ", ".join(str(b) for b in missing[:5]) + more
                         + " (give them in --capacities, read totalBytes from a kafka-log-dirs --sizes document or set --default-capacity)")
    if any(not 0 <= c < 1 << 64 for c in out):
        raise ValueError("capacity: a capacity must be 0..2^64-1")
    return np.array(out, dtype=np.uint64), np.array([c * int(max_utilisation) // 100 for c in out], dtype=np.uint64)


def wave_utilisation(wi: WaveInput, size: np.ndarray, wave: np.ndarray, n_waves: int, stored, capacity) -> List[int]:
    """Per wave: the highest (occ + arr) / capacity in ppm over the brokers that receive bytes in it (0 when none does); occ
    follows the waves, departures counted after their wave."""
    occ = [int(v) for v in stored]
    moves: Dict[int, List[Tuple[int, int, int]]] = {}
    for i in range(len(wi.keys)):
        w, sz = int(wave[i]), int(size[i])
        if w < 0 or sz == 0:
            continue
        cs = {int(b) for b in wi.current[i] if b != NONE}
        ts = {int(b) for b in wi.target[i] if b != NONE}
        moves.setdefault(w, []).extend([(b, sz, 0) for b in ts - cs] + [(b, 0, sz) for b in cs - ts])
    peaks = []
    for w in range(n_waves):
        arr: Dict[int, int] = {}
        for b, a, _ in moves.get(w, []):
            arr[b] = arr.get(b, 0) + a
        peaks.append(max([_ppm(occ[b] + a, capacity[b]) if int(capacity[b]) else 10 ** 6 for b, a in arr.items() if a], default=0))
        for b, a, d in moves.get(w, []):
            occ[b] += a - d
    return peaks


def plan_waves(current_doc: dict, plan_doc: dict, max_per_broker: int = 0, seed: int = 1, *, sizes=None, max_bytes_per_broker: int = 0,
               default_size: Optional[int] = None, capacity: Optional[dict] = None, stored=None, max_utilisation: int = 100,
               default_capacity: Optional[int] = None, headroom: bool = False) -> WavePlan:
    """Split `plan_doc` (relative to `current_doc`) into waves of at most `max_per_broker` movements per broker.  With `sizes`
    ({(topic, partition): bytes}, e.g. from parse_sizes; or a kafka-log-dirs / sizes document or text) or `default_size`, the
    split is kao_plan_waves_sized: at most `max_bytes_per_broker` bytes per broker per wave as well (0 = no byte cap, and
    max_per_broker 0 = no count cap).

    With `capacity` ({broker id: bytes}), `default_capacity`, `max_utilisation` below 100 or `headroom=True` the split is
    kao_plan_waves_headroom: no wave fills a broker beyond capacity * max_utilisation // 100, counting what
    it holds plus everything arriving; both caps are then optional.  Capacities come from capacity_for (the mapping, else the
    totalBytes of a kafka-log-dirs `sizes` document, else `default_capacity`), `stored` ({broker id: bytes} or None) from
    stored_for.  Partitions that fit no wave are in plan.stuck (wave -2) and in no wave document."""
    return _run(_prepare(current_doc, plan_doc, max_per_broker, seed, sizes, max_bytes_per_broker, default_size, capacity, stored,
                         max_utilisation, default_capacity, headroom))


@dataclass
class _Prepared:
    """What plan_waves knows before the library is called: the rows, which call it will be and that call's arrays."""
    input: WaveInput
    call: str                                    # "plain", "sized" or "headroom"
    max_per_broker: int
    max_bytes_per_broker: int
    seed: int
    size: Optional[np.ndarray] = None            # [P] uint64 (sized and headroom)
    stored: Optional[np.ndarray] = None          # [B] uint64 (headroom)
    capacity: Optional[np.ndarray] = None        # [B] uint64 as given, what the utilisation is reported against (headroom)
    effective: Optional[np.ndarray] = None       # [B] uint64 capacity * max_utilisation // 100, what the call takes (headroom)


def _prepare(current_doc, plan_doc, max_per_broker, seed, sizes, max_bytes_per_broker, default_size, capacity, stored, max_utilisation,
             default_capacity, headroom) -> _Prepared:
    """The host-only first step of plan_waves (its arguments, all of them): every ValueError of the inputs is raised here."""
    wi = parse_pair(current_doc, plan_doc)
    headroom = bool(headroom) or capacity is not None or default_capacity is not None or max_utilisation != 100
    sized = headroom or sizes is not None or default_size is not None or max_bytes_per_broker
    pre = _Prepared(wi, "headroom" if headroom else "sized" if sized else "plain", max_per_broker, max_bytes_per_broker, seed)
    if not sized:
        return pre
    dirs = _log_dirs_table(sizes) if headroom else None
    if dirs is not None and sizes is dirs:   # a parse_log_dirs table: a partition's size is its largest non-future replica
        sizes = {}
        for ld in (ld for d in dirs.values() for ld in d.values()):
            for t, p, sz, future in ld.entries:
                if not future:
                    sizes[(t, p)] = max(sizes.get((t, p), 0), sz)
    if sizes is not None and not (isinstance(sizes, dict) and all(isinstance(k, tuple) for k in sizes)):
        sizes = parse_sizes(sizes)
    pre.size = sizes_for(wi, sizes or {}, default_size)
    if headroom:
        pre.capacity, pre.effective = capacity_for(wi, capacity, dirs, default_capacity, max_utilisation)
        pre.stored = stored_for(wi, pre.size, dirs)
        if stored is not None:
            pre.stored = np.array([int(stored.get(int(b), pre.stored[j])) for j, b in enumerate(wi.broker_ids)], dtype=np.uint64)
    return pre


def _run(pre: _Prepared) -> WavePlan:
    """The second step of plan_waves: the one library call, and the WavePlan made of its result."""
    wi, size = pre.input, pre.size
    rows = (wi.current, wi.target, len(wi.broker_ids))
    stats = None
    if pre.call == "headroom":
        wave, nw, lb, stats = plan_waves_headroom_arrays(*rows, size, pre.stored, pre.effective, pre.max_bytes_per_broker,
                                                         pre.max_per_broker, pre.seed)
    elif pre.call == "sized":
        wave, nw, lb = plan_waves_sized_arrays(*rows, size, pre.max_bytes_per_broker, pre.max_per_broker, pre.seed)
    else:
        wave, nw, lb = plan_waves_arrays(*rows, pre.max_per_broker, pre.seed)
    docs = [{"version": 1, "partitions": []} for _ in range(nw)]
    for i, (t, p) in enumerate(wi.keys):
        if wave[i] >= 0:
            docs[int(wave[i])]["partitions"].append({"topic": t, "partition": p, "replicas": wi.target_replicas[i]})
    res = WavePlan(n_waves=nw, lower_bound=lb, optimal=nw == lb, wave=wave, waves=docs, input=wi)
    if size is not None:
        res.size = size
        res.max_broker_bytes, res.bytes_lower_bound = wave_bytes(wi, size, wave, nw, int(pre.max_bytes_per_broker))
    if pre.call == "headroom":
        res.headroom, res.stats = True, stats
        res.stuck = [(wi.keys[i][0], wi.keys[i][1], wi.target_replicas[i]) for i in np.nonzero(wave == -2)[0]]
        res.stuck_bytes = int(stats[1])
        res.stuck_document = {"version": 1, "partitions": [{"topic": t, "partition": p, "replicas": r} for t, p, r in res.stuck]}
        res.optimal = res.optimal and not res.stuck
        res.min_free, res.min_free_wave = int(stats[5]), int(stats[6])
        res.min_free_broker = int(wi.broker_ids[int(stats[7])]) if stats[7] >= 0 else -1
        res.peak_utilisation_ppm = wave_utilisation(wi, size, wave, nw, pre.stored, pre.capacity)
    return res


def parse_bytes(text: str) -> int:
    """A byte count: digits with an optional K / M / G / T suffix (powers of 1024), below 2^64."""
    t = str(text).strip()
    mult = 1
    if t and t[-1].upper() in "KMGT":
        mult = 1024 ** ("KMGT".index(t[-1].upper()) + 1)
        t = t[:-1]
    if not t.isdigit() or int(t) * mult >= 1 << 64:
        raise ValueError(f"not a byte count: {text!r}")
    return int(t) * mult


def main(argv=None) -> int:
    """Python twin of cli/kao-waves: same flags, same files, same exit status (0 ok, 1 error, 2 usage, 3 stuck partitions)."""
    ap = argparse.ArgumentParser(prog="kao-waves", description="split a reassignment plan into waves capped per broker")
    ap.add_argument("--current", required=True)
    ap.add_argument("--plan", required=True)
    ap.add_argument("--max-per-broker", type=int, default=None)
    ap.add_argument("--out-prefix", required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--sizes", default=None, help="kafka-log-dirs --describe output, or {\"partitions\":[{topic,partition,size}]}")
    ap.add_argument("--max-bytes-per-broker", default=None, help="bytes, or with a K/M/G/T suffix (powers of 1024)")
    ap.add_argument("--default-size", default=None, help="bytes of a moving partition --sizes does not list")
    ap.add_argument("--headroom", action="store_true", help="no wave fills a broker beyond its capacity (needs --sizes); stuck partitions "
                    "go to PREFIX-stuck.json and the exit status is 3")
    ap.add_argument("--capacities", default=None, help='{"<brokerId>": bytes} JSON file or id:bytes,id:bytes (implies --headroom)')
    ap.add_argument("--default-capacity", default=None, help="bytes of disk of the brokers without another capacity (implies --headroom)")
    ap.add_argument("--max-utilisation", type=int, default=None, help="fill a broker to at most PCT percent, 1..100 (implies --headroom)")
    a = ap.parse_args(argv)
    headroom = a.headroom or a.capacities is not None or a.default_capacity is not None or a.max_utilisation is not None
    sized = headroom or a.sizes is not None or a.max_bytes_per_broker is not None or a.default_size is not None
    cap_bytes, default_size, default_capacity = 0, None, None
    if headroom and a.sizes is None:
        ap.error("--headroom needs --sizes")
    if a.max_utilisation is not None and not 1 <= a.max_utilisation <= 100:
        ap.error("--max-utilisation needs a percentage 1..100")
    try:
        if a.default_capacity is not None:
            default_capacity = parse_bytes(a.default_capacity)
        if a.max_bytes_per_broker is not None:
            cap_bytes = parse_bytes(a.max_bytes_per_broker)
        if a.default_size is not None:
            default_size = parse_bytes(a.default_size)
            if default_size > MAX_SIZE:
                raise ValueError(f"--default-size above 2^53: {a.default_size}")
    except ValueError as e:
        ap.error(str(e))
    if not sized and a.max_per_broker is None:
        ap.error("the following arguments are required: --max-per-broker")
    if headroom and (a.max_per_broker or 0) < 0:
        ap.error("--max-per-broker must be >= 0")
    if sized and not headroom and ((a.max_per_broker or 0) < 0 or (not a.max_per_broker and cap_bytes == 0)):
        ap.error("give --max-per-broker K >= 1 or --max-bytes-per-broker N >= 1 (K = 0: no count cap)")
    try:
        with open(a.current) as f:
            cur = json.load(f)
        with open(a.plan) as f:
            plan = json.load(f)
        sizes, capacity = ({} if sized else None), None   # a byte flag without --sizes is still the sized call
        if a.sizes is not None:
            with open(a.sizes) as f:
                sizes = f.read()
        if headroom:
            from .disk import _capacities
            capacity = _capacities(a.capacities) if a.capacities is not None else {}
        # a missing size, then a broker without a capacity, are reported here, before the device is touched
        pre = _prepare(cur, plan, a.max_per_broker or 0, a.seed, sizes, cap_bytes, default_size, capacity, None,
                       100 if a.max_utilisation is None else a.max_utilisation, default_capacity, headroom)
        from .solver import init
        init(a.device)
        res = _run(pre)
        for w, doc in enumerate(res.waves):
            with open(f"{a.out_prefix}{w + 1}.json", "w") as f:
                f.write(json.dumps(doc) + "\n")
        if res.stuck:
            with open(f"{a.out_prefix}-stuck.json", "w") as f:
                f.write(json.dumps(res.stuck_document) + "\n")
    except Exception as e:  # noqa: BLE001 -- reported, exit status 1
        print(f"kao-waves: {e}", file=sys.stderr)
        return 1
    if a.report:
        sizes = ",".join(str(len(d["partitions"])) for d in res.waves)
        extra = ""
        if sized:
            extra = (f" bytes_lower_bound={res.bytes_lower_bound} max_broker_bytes_per_wave="
                     + ",".join(str(v) for v in res.max_broker_bytes))
        if headroom:   # the fullest receiving broker of each wave, in percent of its capacity
            extra += (" fullest_receiver_pct_per_wave=" + ",".join(f"{v // 10000}.{v // 100 % 100:02d}" for v in res.peak_utilisation_ppm)
                      + f" min_free={res.min_free} min_free_wave={res.min_free_wave + 1 if res.min_free_wave >= 0 else 0}"
                      f" min_free_broker={res.min_free_broker} stuck={len(res.stuck)} stuck_bytes={res.stuck_bytes}")
        print(f"waves={res.n_waves} lower_bound={res.lower_bound} optimal={'yes' if res.optimal else 'no'} "
              f"partitions_per_wave={sizes}{extra}", file=sys.stderr)
    if res.stuck:
        print(f"stuck: {len(res.stuck)} partitions, {res.stuck_bytes} bytes", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())
