"""Failover-aware follower order: the order of each partition's followers that keeps the peak leader count after a broker or a rack
failure as low as it can be, with the fewest follower swaps (kao_failover_order).

    python -m kafka_assignment_optimizer_amd.failover --current current.json --broker-list 0,1,2 --racks racks.json --scope rack \
        --out plan.json --report

When a broker or a rack goes down Kafka hands each orphaned partition to the first live replica of its list.  The plan holds only
the partitions whose followers change places; every row is the current row with two followers swapped, so executing it moves no
data and changes no preferred leader (kao-waves puts the whole plan in one wave).  The rows of all topics are taken together over
one broker index: the load a failure shifts is a cluster quantity.  Balance the preferred leaders first (kao-leaders), then run
this.  The answer is exact per scenario: peak_after is the lowest peak any follower order reaches, reordered the fewest swaps that
reach it.

`--traffic FILE` or `--sizes FILE` weighs every partition instead (kao_failover_order_weighted): the peak is
the traffic a surviving broker leads after the failure, every scenario runs a deterministic descent, and a lower bound computed
beside it proves the scenario's peak optimal where the two meet.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._plan_args import _racks, count, dense_rows, u64, weight_arg, weight_buffer
from .model import NONE, Topic
from .solver import STATUS_NAMES, _check

STAT_KEYS = ("scenarios", "probes", "phases", "rounds", "paths", "longest_path", "launches", "largest_scenario")
SCEN_KEYS = ("affected", "offline", "peak_before", "peak_after", "reordered")
WEIGHTED_STAT_KEYS = ("scenarios", "rounds", "moves", "proposals", "launches", "stopped_by_max_rounds", "proven_scenarios", "most_rounds")
WEIGHTED_SCEN_KEYS = ("affected", "offline", "peak_before", "peak_after", "lower_bound", "reordered")
SCOPES = {"broker": 0, "rack": 1, 0: 0, 1: 1}


@dataclass
class FailoverResult:
    rows: np.ndarray         # [P, width] uint16: the input rows, e(p) swapped with the chosen slot (the input rows with dry_run)
    scen: np.ndarray         # [n_scen, 5] int32, see SCEN_KEYS; n_scen = n_brokers (scope 0) or n_racks (scope 1)
    n_reordered: int         # rows that changed (would change with dry_run): the sum of scen[:, 4]
    stats: np.ndarray        # int32[8], see STAT_KEYS / include/kao.h


@dataclass
class WeightedFailoverResult:
    rows: np.ndarray         # [P, width] uint16: the input rows, e(p) swapped with the chosen slot (the input rows with dry_run)
    scen: np.ndarray         # [n_scen, 6] uint64, see WEIGHTED_SCEN_KEYS
    n_reordered: int         # rows that changed (would change with dry_run): the sum of scen[:, 5]
    status: str              # "OPTIMAL_PROVEN" (peak_after == lower_bound in every scenario) | "FEASIBLE_BOUND_GAP"
    stats: np.ndarray        # int64[8], see WEIGHTED_STAT_KEYS / include/kao.h


@dataclass
class FailoverInput:
    """A cluster as rows over one broker index."""
    keys: List[Tuple[str, int]]   # (topic, partition) per row
    broker_ids: np.ndarray        # dense index -> broker id
    rack_of: np.ndarray           # [B] dense rack index
    rack_names: List[str]         # rack index -> name
    rows: np.ndarray              # [P, width] uint16 dense, NONE-padded


@dataclass
class FailoverPlan:
    result: FailoverResult        # a WeightedFailoverResult from the weighted entry points
    input: FailoverInput
    scope: int
    weight: Optional[np.ndarray] = None   # [P] uint64 per row (weighted plans)
    entries: List[Tuple[str, int, List[int]]] = field(default_factory=list)   # (topic, partition, replicas as broker ids) of the reordered rows
    assignments: Optional[List[np.ndarray]] = None                           # per topic, when topics were given


def _scope(scope) -> int:
    if scope not in SCOPES:
        raise ValueError(f"scope must be 'broker' (0) or 'rack' (1), got {scope!r}")
    return SCOPES[scope]


def _rack_buffer(rack_of, n_brokers) -> np.ndarray:
    rk = np.ascontiguousarray(rack_of, dtype=np.uint8)
    if rk.shape != (int(n_brokers),):
        raise ValueError(f"rack_of must hold one rack per broker ({n_brokers}), got shape {rk.shape}")
    return rk


def failover_order_arrays(rows, n_brokers: int, rack_of, n_racks: int, scope, dry_run: bool = False) -> FailoverResult:
    """kao_failover_order on dense rows ([P, width], NONE-padded, slot 0 = preferred leader)."""
    scope = _scope(scope)
    r, flat, P, W = dense_rows(rows)
    rk = _rack_buffer(rack_of, n_brokers)
    n_scen = int(n_brokers) if scope == 0 else int(n_racks)
    scen = np.zeros((max(n_scen, 1), 5), dtype=np.int32)
    stats = np.zeros(8, dtype=np.int32)
    n = C.c_int32(0)
    i32 = C.POINTER(C.c_int32)
    _check(_ffi.load().kao_failover_order(int(n_brokers), int(n_racks), rk.ctypes.data_as(C.POINTER(C.c_uint8)), int(P), int(W),
                                          flat.ctypes.data_as(C.POINTER(C.c_uint16)), scope, int(bool(dry_run)), scen.ctypes.data_as(i32),
                                          C.byref(n), stats.ctypes.data_as(i32)), "kao_failover_order")
    return FailoverResult(rows=r, scen=scen[:n_scen], n_reordered=int(n.value), stats=stats)


def failover_order_weighted_arrays(rows, n_brokers: int, rack_of, n_racks: int, scope, weight, min_gain: int = 0, max_rounds: int = 0,
                                   dry_run: bool = False) -> WeightedFailoverResult:
    """kao_failover_order_weighted on dense rows ([P, width], NONE-padded, slot 0 = preferred leader); weight[p] is the traffic of
    row p."""
    scope = _scope(scope)
    r, flat, P, W = dense_rows(rows)
    rk = _rack_buffer(rack_of, n_brokers)
    wbuf = weight_buffer(weight, P, min_gain)
    n_scen = int(n_brokers) if scope == 0 else int(n_racks)
    scen = np.zeros((max(n_scen, 1), 6), dtype=np.uint64)
    stats = np.zeros(8, dtype=np.int64)
    n, status = C.c_int32(0), C.c_int32(0)
    _check(_ffi.load().kao_failover_order_weighted(int(n_brokers), int(n_racks), rk.ctypes.data_as(C.POINTER(C.c_uint8)), int(P), int(W),
                                                   flat.ctypes.data_as(C.POINTER(C.c_uint16)), wbuf.ctypes.data_as(C.POINTER(C.c_uint64)), scope,
                                                   int(min_gain), int(max_rounds), int(bool(dry_run)), scen.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   C.byref(n), C.byref(status), stats.ctypes.data_as(C.POINTER(C.c_int64))),
           "kao_failover_order_weighted")
    return WeightedFailoverResult(rows=r, scen=scen[:n_scen], n_reordered=int(n.value), status=STATUS_NAMES[int(status.value)], stats=stats)


def parse_current(doc: dict, broker_list: Sequence[int], racks: dict) -> FailoverInput:
    """A reassignment document as rows over `broker_list` (dense index = position), partitions ordered by (topic, partition).
    Every replica must be a broker of the list: a failure of a broker outside it cannot be described."""
    ids = [int(b) for b in broker_list]
    if not ids:
        raise ValueError("empty broker list")
    dense = {}
    for i, b in enumerate(ids):
        if b in dense:
            raise ValueError("duplicate id in broker list")
        dense[b] = i
    names = []
    for b in ids:
        if b not in racks:
            raise ValueError(f"no rack given for broker {b}")
        names.append(str(racks[b]))
    rack_names = sorted(set(names))
    rack_idx = {n: i for i, n in enumerate(rack_names)}
    parts = doc.get("partitions")
    if not isinstance(parts, list):
        raise ValueError('missing "partitions" array')
    by_key = {}
    for e in parts:
        by_key[(str(e["topic"]), int(e["partition"]))] = [int(b) for b in e["replicas"]]
    keys = sorted(by_key)
    width = max([1] + [len(by_key[k]) for k in keys])
    rows = np.full((len(keys), width), NONE, dtype=np.uint16)
    for i, k in enumerate(keys):
        reps = by_key[k]
        if not reps:
            raise ValueError(f"partition {k[0]}-{k[1]} has no replica")
        for j, b in enumerate(reps):
            if b not in dense:
                raise ValueError(f"partition {k[0]}-{k[1]} has a replica outside --broker-list (broker {b})")
            rows[i, j] = dense[b]
    return FailoverInput(keys=keys, broker_ids=np.array(ids, dtype=np.int64), rack_of=np.array([rack_idx[n] for n in names], dtype=np.uint8),
                         rack_names=rack_names, rows=rows)


def _from_topics(topics: Sequence[Topic], assignments) -> FailoverInput:
    t0 = topics[0]
    for t in topics:
        if not (np.array_equal(t.broker_ids, t0.broker_ids) and np.array_equal(t.rack_of, t0.rack_of) and t.n_racks == t0.n_racks):
            raise ValueError(f"topic {t.name}: all topics must share one broker index (broker_ids, rack_of, n_racks)")
    given = [t.current for t in topics] if assignments is None else list(assignments)
    if len(given) != len(topics):
        raise ValueError("one assignment per topic")
    given = [np.asarray(a, dtype=np.uint16).reshape(t.n_partitions, -1) for t, a in zip(topics, given)]
    width = max(a.shape[1] for a in given)
    rows = np.full((sum(t.n_partitions for t in topics), width), NONE, dtype=np.uint16)
    keys, at = [], 0
    for t, a in zip(topics, given):
        rows[at:at + t.n_partitions, :a.shape[1]] = a
        pids = range(t.n_partitions) if t.partition_ids is None else [int(x) for x in t.partition_ids]
        keys += [(t.name, int(p)) for p in pids]
        at += t.n_partitions
    return FailoverInput(keys=keys, broker_ids=np.asarray(t0.broker_ids, dtype=np.int64), rack_of=np.asarray(t0.rack_of, dtype=np.uint8),
                         rack_names=[str(r) for r in range(t0.n_racks)], rows=rows)


def failover_order(topics_or_doc, scope, dry_run: bool = False, *, broker_list=None, racks=None, assignments=None) -> FailoverPlan:
    """kao_failover_order on a whole cluster: a list of Topic that share one broker index (rows = `assignments`, default each
    topic's current; topics of different RF are padded), or a reassignment document with `broker_list` and `racks`
    ({broker id: rack name})."""
    scope = _scope(scope)
    topics = None
    if isinstance(topics_or_doc, dict):
        if broker_list is None or racks is None:
            raise ValueError("a reassignment document needs broker_list and racks")
        fi = parse_current(topics_or_doc, broker_list, racks)
    else:
        topics = list(topics_or_doc)
        if not topics:
            raise ValueError("no topic given")
        fi = _from_topics(topics, assignments)
    plan = plan_input(fi, scope, dry_run)
    if topics is not None:
        plan.assignments, at = [], 0
        for i, t in enumerate(topics):
            w = t.current.shape[1] if assignments is None else np.asarray(assignments[i]).reshape(t.n_partitions, -1).shape[1]
            plan.assignments.append(plan.result.rows[at:at + t.n_partitions, :w].copy())
            at += t.n_partitions
    return plan


def plan_input(fi: FailoverInput, scope, dry_run: bool = False) -> FailoverPlan:
    """kao_failover_order on a FailoverInput; the entries are the rows that changed (none with dry_run: the rows stay as they are)."""
    scope = _scope(scope)
    res = failover_order_arrays(fi.rows, len(fi.broker_ids), fi.rack_of, len(fi.rack_names), scope, dry_run)
    changed = np.nonzero((res.rows != fi.rows).any(axis=1))[0]
    entries = [(fi.keys[p][0], fi.keys[p][1], [int(fi.broker_ids[b]) for b in res.rows[p] if b != NONE]) for p in changed]
    return FailoverPlan(result=res, input=fi, scope=scope, entries=entries)


def plan_input_weighted(fi: FailoverInput, scope, weight, min_gain: int = 0, max_rounds: int = 0, dry_run: bool = False) -> FailoverPlan:
    """kao_failover_order_weighted on a FailoverInput, weight[p] per row of it; the entries are the rows that changed."""
    scope = _scope(scope)
    res = failover_order_weighted_arrays(fi.rows, len(fi.broker_ids), fi.rack_of, len(fi.rack_names), scope, weight, min_gain, max_rounds, dry_run)
    changed = np.nonzero((res.rows != fi.rows).any(axis=1))[0]
    entries = [(fi.keys[p][0], fi.keys[p][1], [int(fi.broker_ids[b]) for b in res.rows[p] if b != NONE]) for p in changed]
    return FailoverPlan(result=res, input=fi, scope=scope, weight=np.asarray(weight, dtype=np.uint64), entries=entries)


def failover_order_weighted(topics_or_doc, scope, weights, min_gain: int = 0, max_rounds: int = 0, dry_run: bool = False, *, broker_list=None,
                            racks=None, assignments=None, default_weight: Optional[int] = None) -> FailoverPlan:
    """kao_failover_order_weighted on a whole cluster, given as for failover_order.  `weights` is {(topic name, partition id): weight}
    (partitions it does not name take `default_weight`; without one they are an error) or, with topics, one array per topic."""
    from .leaders import weights_for
    scope = _scope(scope)
    topics = None
    if isinstance(topics_or_doc, dict):
        if broker_list is None or racks is None:
            raise ValueError("a reassignment document needs broker_list and racks")
        fi = parse_current(topics_or_doc, broker_list, racks)
    else:
        topics = list(topics_or_doc)
        if not topics:
            raise ValueError("no topic given")
        if len({t.name for t in topics}) != len(topics):
            raise ValueError("topic names must be distinct")
        fi = _from_topics(topics, assignments)
    if isinstance(weights, dict):
        weight = weights_for(fi.keys, weights, default_weight)
    else:
        per = [np.asarray(w).reshape(-1) for w in weights]
        if topics is None or len(per) != len(topics) or any(len(w) != t.n_partitions for w, t in zip(per, topics)):
            raise ValueError("weights: a table, or with topics one array of n_partitions values per topic")
        weight = np.concatenate(per)
    plan = plan_input_weighted(fi, scope, weight, min_gain, max_rounds, dry_run)
    if topics is not None:
        plan.assignments, at = [], 0
        for i, t in enumerate(topics):
            w = t.current.shape[1] if assignments is None else np.asarray(assignments[i]).reshape(t.n_partitions, -1).shape[1]
            plan.assignments.append(plan.result.rows[at:at + t.n_partitions, :w].copy())
            at += t.n_partitions
    return plan


def weighted_report_lines(plan: FailoverPlan) -> List[str]:
    """The --traffic / --sizes --report text, line for line as cli/kao-failover prints it."""
    fi, res = plan.input, plan.result
    scen, s = [[int(x) for x in row] for row in res.scen.tolist()], res.stats
    out = []
    for g, (aff, off, before, after, bound, re_) in enumerate(scen):
        if aff or off:
            name = str(int(fi.broker_ids[g])) if plan.scope == 0 else fi.rack_names[g]
            out.append(f"scenario={name} affected={aff} offline={off} peak_before={before} peak_after={after} lower_bound={bound} reordered={re_}")
    out.append(f"weighted: scope={'broker' if plan.scope == 0 else 'rack'} scenarios={len(scen)} worst_peak_before={max(r[2] for r in scen)} "
               f"worst_peak_after={max(r[3] for r in scen)} worst_lower_bound={max(r[4] for r in scen)} proven={s[6]} "
               f"offline={sum(r[1] for r in scen)} reordered={res.n_reordered} rounds={s[1]} moves={s[2]} launches={s[4]}")
    return out


def report_lines(plan: FailoverPlan) -> List[str]:
    """The --report text, line for line as cli/kao-failover prints it."""
    fi, scen = plan.input, plan.result.scen
    out = []
    for g, (aff, off, before, after, re) in enumerate(scen.tolist()):
        if aff or off:
            name = str(int(fi.broker_ids[g])) if plan.scope == 0 else fi.rack_names[g]
            out.append(f"scenario={name} affected={aff} offline={off} peak_before={before} peak_after={after} reordered={re}")
    out.append(f"scope={'broker' if plan.scope == 0 else 'rack'} scenarios={len(scen)} worst_peak_before={int(scen[:, 2].max())} "
               f"worst_peak_after={int(scen[:, 3].max())} offline={int(scen[:, 1].sum())} reordered={plan.result.n_reordered}")
    return out


def main(argv=None) -> int:
    """Python twin of cli/kao-failover: same flags, same bytes, same exit status (0 ok, 1 error, 2 usage)."""
    from .leaders import parse_traffic, plan_text, weights_for
    ap = argparse.ArgumentParser(prog="kao-failover", description="follower order that keeps the peak leader count after a failure lowest; moves no data")
    ap.add_argument("--current", required=True, help="reassignment JSON of the cluster as it is")
    ap.add_argument("--broker-list", required=True, help="brokers of the cluster, CSV")
    ap.add_argument("--racks", required=True, help='{"<brokerId>": "<rack>"} JSON file or id:rack,id:rack')
    ap.add_argument("--scope", required=True, choices=["broker", "rack"], help="failures to prepare for: single brokers or whole racks")
    ap.add_argument("--dry-run", action="store_true", help="report only: the plan stays empty")
    ap.add_argument("--out", default="")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--device", type=int, default=0)

    ap.add_argument("--traffic", default=None, help='weigh the partitions: {"version":1,"partitions":[{"topic":..,"partition":..,"weight":N}]}')
    ap.add_argument("--sizes", default=None, help="weigh the partitions by their size: kafka-log-dirs --describe output")
    ap.add_argument("--default-weight", type=weight_arg, default=None, help="weight of the partitions the file does not name")
    ap.add_argument("--min-gain", type=u64, default=None, help="weighted: an heir changes only when that closes a gap of more than N")
    ap.add_argument("--max-rounds", type=count, default=None, help="weighted: stop every scenario after N rounds")
    a = ap.parse_args(argv)
    weighted = a.traffic is not None or a.sizes is not None
    if a.traffic is not None and a.sizes is not None:
        ap.error("give one of --traffic and --sizes")
    if not weighted and (a.default_weight is not None or a.min_gain is not None or a.max_rounds is not None):
        ap.error("--default-weight, --min-gain and --max-rounds need --traffic or --sizes")
    try:
        with open(a.current) as f:
            doc = json.load(f)
        fi = parse_current(doc, [int(b) for b in a.broker_list.split(",") if b], _racks(a.racks))   # input errors before the device is touched
        if weighted:
            if a.traffic is not None:
                with open(a.traffic) as f:
                    table = parse_traffic(json.load(f))
            else:
                from .waves import parse_sizes
                with open(a.sizes) as f:
                    table = parse_sizes(f.read())
            weight = weights_for(fi.keys, table, a.default_weight)
        from .solver import init
        init(a.device)
        if weighted:
            plan = plan_input_weighted(fi, a.scope, weight, a.min_gain or 0, a.max_rounds or 0, a.dry_run)
        else:
            plan = plan_input(fi, a.scope, a.dry_run)
        if a.report:
            for line in weighted_report_lines(plan) if weighted else report_lines(plan):
                print(line, file=sys.stderr)
        text = plan_text(plan.entries)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        else:
            sys.stdout.write(text)
    except Exception as e:  # noqa: BLE001 -- reported, exit status 1
        print(f"kao-failover: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
