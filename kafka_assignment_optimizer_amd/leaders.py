"""Leader-only rebalancing: the fewest preferred-leader changes that put every broker inside the leader band, replica sets kept
(kao_balance_leaders).

    python -m kafka_assignment_optimizer_amd.leaders --current current.json --broker-list 0,1,2 --racks racks.json --out plan.json

writes a reassignment document that holds only the partitions whose preferred leader changes; every row is the current row with
the new leader swapped to the front, so `kafka-reassign-partitions --execute` moves no data (kao-waves puts the whole plan in one
wave).  Topics are balanced one by one: the band is floor / ceil of partitions / brokers per topic, `--slack N` widens it by N on
both sides, `--auto-slack` takes the smallest N that is feasible.  The answer is exact: n_changed is the proven minimum, or the
topic is proven infeasible (no choice of leaders among its replicas meets the band).

`--cluster` balances the leaders of all topics together instead (kao_balance_leaders_cluster): every topic
keeps its band, and the largest number of partitions any broker leads over the whole cluster is made as low as leader changes alone
can make it (or held to `--cluster-hi N`), every broker leading at least `--cluster-lo N`, with the fewest changes.

`--traffic FILE` or `--sizes FILE` weighs every partition instead (kao_balance_leaders_weighted): the traffic a
broker leads is made even by a deterministic descent over all topics together, and a lower bound computed beside it proves the peak
optimal where the two meet (status OPTIMAL_PROVEN; FEASIBLE_BOUND_GAP otherwise, exit status 0 both times).  `--exchange` goes on
from the state where no single leader change helps: two partitions that share a broker pair swap their leaders
(kao_balance_leaders_weighted_exchange).  No data moves either way: the peak is never higher than without the
flag, the election list is longer.
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _ffi
from ._plan_args import MAX_WEIGHT, _racks, count, dense_rows, u64, weight_arg, weight_buffer
from .model import NONE, Topic, topics_from_json
from .solver import STATUS_NAMES, _check, _CTopics

CLUSTER_STAT_KEYS = ("probes", "phases", "rounds", "paths", "longest_path", "launches", "pair_nodes", "unrouted")
WEIGHTED_STAT_KEYS = ("rounds", "moves", "proposals", "launches", "single_workgroup", "stopped_by_max_rounds", "level_k", "leading_brokers")
# kao_balance_leaders_weighted_exchange: rounds, moves and proposals count both kinds of round
WEIGHTED_X_STAT_KEYS = WEIGHTED_STAT_KEYS + ("exchange_rounds", "exchanges", "exchange_proposals", "pair_index_entries")
STAT_KEYS = ("phases", "rounds", "paths", "longest_path", "over_before", "under_before", "launches", "unrouted")


@dataclass
class LeaderResult:
    assignment: np.ndarray   # [P, rf] uint16: the input rows, slot 0 swapped with the chosen leader's slot (untouched when infeasible)
    n_changed: int           # partitions whose preferred leader changed: the minimum
    objective: int           # README objective of `assignment` against topic.current (K-eval)
    status: str              # "OPTIMAL_PROVEN" | "INFEASIBLE_PROVEN"
    stats: np.ndarray        # int32[8], see STAT_KEYS / include/kao.h


def balance_leaders(topic: Topic, assignment=None) -> LeaderResult:
    """kao_balance_leaders on one topic.  `assignment` ([P, rf], complete rows) defaults to topic.current, which then needs
    rf == rf_cur.  The leader band is topic.bounds_override's lead_lo / lead_hi, else floor / ceil of P / B."""
    if assignment is None:
        if topic.rf != topic.rf_cur:
            raise ValueError(f"topic {topic.name}: rf {topic.rf} != rf_cur {topic.rf_cur}; pass the assignment to balance")
        assignment = topic.current
    a = np.ascontiguousarray(assignment, dtype=np.uint16).reshape(-1).copy()
    if a.size != topic.n_partitions * topic.rf:
        raise ValueError("assignment must have P*rf entries")
    ct = _CTopics([topic])
    n, status, obj = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    stats = np.zeros(8, dtype=np.int32)
    _check(_ffi.load().kao_balance_leaders(ct.arr, a.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(n), C.byref(obj), C.byref(status),
                                           stats.ctypes.data_as(C.POINTER(C.c_int32))), "kao_balance_leaders")
    return LeaderResult(assignment=a.reshape(topic.n_partitions, topic.rf), n_changed=int(n.value), objective=int(obj.value),
                        status=STATUS_NAMES[int(status.value)], stats=stats)


def _with_slack(topic: Topic, slack: int) -> Topic:
    lo, hi = topic.n_partitions // topic.n_brokers, -(-topic.n_partitions // topic.n_brokers)
    return dataclasses.replace(topic, bounds_override={**topic.bounds_override, "lead_lo": max(0, lo - slack), "lead_hi": hi + slack})


def balance_topic(topic: Topic, slack: int = 0, auto_slack: bool = False):
    """(LeaderResult, slack used): the band widened by `slack`; with auto_slack by the smallest N >= slack that is feasible."""
    while True:
        res = balance_leaders(_with_slack(topic, slack))
        if res.status == "OPTIMAL_PROVEN" or not auto_slack or slack > topic.n_partitions:
            return res, slack
        slack += 1


@dataclass
class ClusterLeaderResult:
    rows: np.ndarray         # [P, width] uint16: the input rows, slot 0 swapped with the chosen leader's slot (untouched with dry_run / infeasible)
    n_changed: int           # partitions whose preferred leader changes: the minimum at peak_after
    peak_before: int         # the most partitions a broker leads, over all topics, in the input
    peak_after: int          # ... in the chosen rows: the lowest reachable with cluster_hi = -1
    status: str              # "OPTIMAL_PROVEN" | "INFEASIBLE_PROVEN"
    stats: np.ndarray        # int32[8], see CLUSTER_STAT_KEYS / include/kao.h


@dataclass
class ClusterLeaderPlan:
    result: ClusterLeaderResult
    keys: List[Tuple[str, int]]                                                # (topic, partition) per row
    entries: List[Tuple[str, int, List[int]]] = field(default_factory=list)   # (topic, partition, replicas as broker ids) of the changed rows
    assignments: Optional[List[np.ndarray]] = None                            # per topic, when topics were given


def balance_leaders_cluster_arrays(rows, n_brokers: int, topic_of, topic_lo, topic_hi, cluster_lo: int = 0, cluster_hi: int = -1,
                                   dry_run: bool = False) -> ClusterLeaderResult:
    """kao_balance_leaders_cluster on dense rows ([P, width], NONE-padded, slot 0 = preferred leader) of all topics over one
    broker index; topic_of[p] is the topic of row p, topic_lo / topic_hi the topics' bands."""
    r, flat, P, W = dense_rows(rows)
    tof = np.ascontiguousarray(topic_of, dtype=np.int32).reshape(-1)
    if tof.shape != (P,):
        raise ValueError(f"topic_of must hold one topic per row ({P}), got {tof.shape[0]}")
    tlo = np.ascontiguousarray(topic_lo, dtype=np.int32).reshape(-1)
    thi = np.ascontiguousarray(topic_hi, dtype=np.int32).reshape(-1)
    if tlo.shape != thi.shape:
        raise ValueError("topic_lo and topic_hi must have one entry per topic each")
    tof_buf = tof if P else np.zeros(1, dtype=np.int32)
    n, before, after, status = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    stats = np.zeros(8, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    _check(_ffi.load().kao_balance_leaders_cluster(int(n_brokers), int(P), int(W), flat.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                   tof_buf.ctypes.data_as(i32), int(tlo.shape[0]), tlo.ctypes.data_as(i32), thi.ctypes.data_as(i32),
                                                   int(cluster_lo), int(cluster_hi), int(bool(dry_run)), C.byref(n), C.byref(before),
                                                   C.byref(after), C.byref(status), stats.ctypes.data_as(i32)), "kao_balance_leaders_cluster")
    return ClusterLeaderResult(rows=r, n_changed=int(n.value), peak_before=int(before.value), peak_after=int(after.value),
                               status=STATUS_NAMES[int(status.value)], stats=stats)


def _plan_cluster(keys, rows, broker_ids, n_brokers, slack, cluster_lo, cluster_hi, dry_run) -> ClusterLeaderPlan:
    """The rows of `keys` ((topic, partition), grouped by topic) through kao_balance_leaders_cluster: each topic's band is floor /
    ceil of its partitions / brokers, widened by `slack` on both sides."""
    names, topic_of = [], np.zeros(len(keys), dtype=np.int32)
    for i, (name, _) in enumerate(keys):
        if not names or names[-1] != name:
            names.append(name)
        topic_of[i] = len(names) - 1
    if len(set(names)) != len(names):
        raise ValueError("the rows of a topic must be contiguous")
    sizes = np.bincount(topic_of, minlength=max(len(names), 1))
    tlo = np.maximum(0, sizes // n_brokers - slack)
    thi = -(-sizes // n_brokers) + slack
    res = balance_leaders_cluster_arrays(rows, n_brokers, topic_of, tlo, thi, cluster_lo, cluster_hi, dry_run)
    changed = np.nonzero((res.rows != rows).any(axis=1))[0]
    entries = [(keys[p][0], keys[p][1], [int(broker_ids[b]) for b in res.rows[p] if b != NONE]) for p in changed]
    return ClusterLeaderPlan(result=res, keys=list(keys), entries=entries)


def balance_leaders_cluster(topics: Sequence[Topic], slack: int = 0, cluster_lo: int = 0, cluster_hi: int = -1, dry_run: bool = False,
                            assignments=None) -> ClusterLeaderPlan:
    """kao_balance_leaders_cluster on topics that share one broker index (broker_ids); rows = `assignments`, default each topic's
    current; topics of different RF are padded.  Returns the per-topic assignments and the plan entries of the changed rows."""
    from .failover import _from_topics
    topics = list(topics)
    if not topics:
        raise ValueError("no topic given")
    if slack < 0:
        raise ValueError("slack must be >= 0")
    if len({t.name for t in topics}) != len(topics):
        raise ValueError("topic names must be distinct")
    fi = _from_topics(topics, assignments)
    plan = _plan_cluster(fi.keys, fi.rows, fi.broker_ids, len(fi.broker_ids), slack, cluster_lo, cluster_hi, dry_run)
    plan.assignments, at = [], 0
    for i, t in enumerate(topics):
        w = t.current.shape[1] if assignments is None else np.asarray(assignments[i]).reshape(t.n_partitions, -1).shape[1]
        plan.assignments.append(plan.result.rows[at:at + t.n_partitions, :w].copy())
        at += t.n_partitions
    return plan


def cluster_report_line(res: ClusterLeaderResult) -> str:
    """The --cluster --report text, as cli/kao-leaders prints it."""
    s = res.stats
    return (f"cluster: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} leader_changes={res.n_changed} "
            f"probes={s[0]} phases={s[1]} rounds={s[2]} paths={s[3]} longest_path={s[4]} launches={s[5]} pair_nodes={s[6]} unrouted={s[7]}")


@dataclass
class WeightedLeaderResult:
    rows: np.ndarray         # [P, width] uint16: the input rows, slot 0 swapped with the chosen leader's slot (untouched with dry_run)
    n_changed: int           # partitions whose preferred leader changes
    peak_before: int         # the largest weight a broker leads in the input
    peak_after: int          # ... in the chosen rows; never above peak_before
    lower_bound: int         # no choice of leaders has a peak below it
    status: str              # "OPTIMAL_PROVEN" (peak_after == lower_bound) | "FEASIBLE_BOUND_GAP"
    stats: np.ndarray        # int64[8], see WEIGHTED_STAT_KEYS / include/kao.h; int64[12], WEIGHTED_X_STAT_KEYS, with exchange
    exchange: bool = False   # the call was kao_balance_leaders_weighted_exchange
    exchange_rounds: int = 0 # stats[8]: rounds that swapped the leaders of two partitions
    exchanges: int = 0       # stats[9]: such swaps applied


@dataclass
class WeightedLeaderPlan:
    result: WeightedLeaderResult
    keys: List[Tuple[str, int]]                                                # (topic, partition) per row
    weight: np.ndarray                                                         # [P] uint64
    entries: List[Tuple[str, int, List[int]]] = field(default_factory=list)   # (topic, partition, replicas as broker ids) of the changed rows
    assignments: Optional[List[np.ndarray]] = None                            # per topic, when topics were given


def balance_leaders_weighted_arrays(rows, n_brokers: int, weight, min_gain: int = 0, max_rounds: int = 0,
                                    dry_run: bool = False, exchange: bool = False) -> WeightedLeaderResult:
    """kao_balance_leaders_weighted on dense rows ([P, width], NONE-padded, slot 0 = preferred leader) of all topics over one
    broker index; weight[p] is the traffic of row p.  exchange=True calls kao_balance_leaders_weighted_exchange: exchange rounds
    follow when no move is left; stats is int64[12]."""
    r, flat, P, W = dense_rows(rows)
    wbuf = weight_buffer(weight, P, min_gain)
    n, status = C.c_int32(0), C.c_int32(0)
    before, after, bound = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    stats = np.zeros(12 if exchange else 8, dtype=np.int64)
    name = "kao_balance_leaders_weighted_exchange" if exchange else "kao_balance_leaders_weighted"
    _check(getattr(_ffi.load(), name)(int(n_brokers), int(P), int(W), flat.ctypes.data_as(C.POINTER(C.c_uint16)),
                                      wbuf.ctypes.data_as(C.POINTER(C.c_uint64)), int(min_gain), int(max_rounds), int(bool(dry_run)),
                                      C.byref(n), C.byref(before), C.byref(after), C.byref(bound), C.byref(status),
                                      stats.ctypes.data_as(C.POINTER(C.c_int64))), name)
    return WeightedLeaderResult(rows=r, n_changed=int(n.value), peak_before=int(before.value), peak_after=int(after.value),
                                lower_bound=int(bound.value), status=STATUS_NAMES[int(status.value)], stats=stats, exchange=bool(exchange),
                                exchange_rounds=int(stats[8]) if exchange else 0, exchanges=int(stats[9]) if exchange else 0)


def _weight_value(v, what):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= MAX_WEIGHT:
        raise ValueError(f"traffic: {what}: weight must be an integer 0..2^53, got {v!r}")
    return v


def parse_traffic(doc) -> Dict[Tuple[str, int], int]:
    """{(topic, partition): weight} from {"version":1,"partitions":[{"topic":..,"partition":..,"weight":N}]}; N is an integer
    0..2^53, a partition listed twice is an error."""
    parts = doc.get("partitions") if isinstance(doc, dict) else None
    if not isinstance(parts, list):
        raise ValueError('traffic: missing "partitions" array')
    out: Dict[Tuple[str, int], int] = {}
    for e in parts:
        if not isinstance(e, dict) or "topic" not in e or "partition" not in e:
            raise ValueError("traffic: partition entry needs topic/partition/weight")
        key = (str(e["topic"]), int(e["partition"]))
        if key in out:
            raise ValueError(f"traffic: partition {key[0]}-{key[1]} listed twice")
        out[key] = _weight_value(e.get("weight"), f"{key[0]}-{key[1]}")
    return out


def weights_for(keys, table: Dict[Tuple[str, int], int], default_weight: Optional[int] = None, what: str = "weight",
                hint: str = "name them in the file or set --default-weight") -> np.ndarray:
    """weight[p] over `keys`.  A partition the table does not name takes `default_weight`; without one it is a ValueError naming
    the first few such partitions (`what` and `hint` word it for the tools that weigh by something else: disk.py)."""
    weight = np.zeros(len(keys), dtype=np.uint64)
    missing = []
    for i, key in enumerate(keys):
        if key in table:
            weight[i] = table[key]
        elif default_weight is None:
            missing.append(f"{key[0]}-{key[1]}")
        else:
            weight[i] = default_weight
    if missing:
        more = f" and {len(missing) - 5} more" if len(missing) > 5 else ""
        raise ValueError(f"no {what} for partitions {', '.join(missing[:5])}{more} ({hint})")
    return weight


def _plan_weighted(keys, rows, broker_ids, weight, min_gain, max_rounds, dry_run, exchange=False) -> WeightedLeaderPlan:
    res = balance_leaders_weighted_arrays(rows, len(broker_ids), weight, min_gain, max_rounds, dry_run, exchange)
    changed = np.nonzero((res.rows != rows).any(axis=1))[0]
    entries = [(keys[p][0], keys[p][1], [int(broker_ids[b]) for b in res.rows[p] if b != NONE]) for p in changed]
    return WeightedLeaderPlan(result=res, keys=list(keys), weight=np.asarray(weight, dtype=np.uint64), entries=entries)


def balance_leaders_weighted(topics: Sequence[Topic], weights, min_gain: int = 0, max_rounds: int = 0, dry_run: bool = False,
                             assignments=None, default_weight: Optional[int] = None, exchange: bool = False) -> WeightedLeaderPlan:
    """kao_balance_leaders_weighted on topics that share one broker index (broker_ids); rows = `assignments`, default each topic's
    current; topics of different RF are padded.  `weights` is {(topic name, partition id): weight} (partitions it does not name
    take `default_weight`) or one array per topic.  exchange=True selects kao_balance_leaders_weighted_exchange.  Returns the
    per-topic assignments and the plan entries of the changed rows."""
    from .failover import _from_topics
    topics = list(topics)
    if not topics:
        raise ValueError("no topic given")
    if len({t.name for t in topics}) != len(topics):
        raise ValueError("topic names must be distinct")
    fi = _from_topics(topics, assignments)
    if isinstance(weights, dict):
        weight = weights_for(fi.keys, weights, default_weight)
    else:
        per = [np.asarray(w).reshape(-1) for w in weights]
        if len(per) != len(topics) or any(len(w) != t.n_partitions for w, t in zip(per, topics)):
            raise ValueError("weights: one array of n_partitions values per topic")
        weight = np.concatenate(per)
    plan = _plan_weighted(fi.keys, fi.rows, fi.broker_ids, weight, min_gain, max_rounds, dry_run, exchange)
    plan.assignments, at = [], 0
    for i, t in enumerate(topics):
        w = t.current.shape[1] if assignments is None else np.asarray(assignments[i]).reshape(t.n_partitions, -1).shape[1]
        plan.assignments.append(plan.result.rows[at:at + t.n_partitions, :w].copy())
        at += t.n_partitions
    return plan


def weighted_report_line(res: WeightedLeaderResult) -> str:
    """The --traffic / --sizes --report text, as cli/kao-leaders prints it: a second line with --exchange."""
    s = res.stats
    line = (f"weighted: status={res.status} peak_before={res.peak_before} peak_after={res.peak_after} lower_bound={res.lower_bound} "
            f"leader_changes={res.n_changed} rounds={s[0]} moves={s[1]} launches={s[3]}")
    return line + (f"\nexchange: rounds={s[8]} exchanges={s[9]} proposals={s[10]} pair_index_entries={s[11]}" if res.exchange else "")


def plan_text(entries) -> str:
    """The reassignment document of [(topic, partition, replicas)], byte for byte as cli/kao-leaders writes it."""
    rows = ['    {"topic":"%s","partition":%d,"replicas":[%s]}' % (t.replace("\\", "\\\\").replace('"', '\\"'), p, ",".join(str(b) for b in r))
            for t, p, r in entries]
    return '{"version":1,"partitions":[' + "".join(("\n" if i == 0 else ",\n") + r for i, r in enumerate(rows)) + "\n]}\n"


def main(argv=None) -> int:
    """Python twin of cli/kao-leaders: same flags, same bytes, same exit status (0 ok, 1 error or infeasible, 2 usage)."""
    ap = argparse.ArgumentParser(prog="kao-leaders", description="fewest preferred-leader changes that balance the leaders; moves no data")
    ap.add_argument("--current", required=True, help="reassignment JSON of the cluster as it is")
    ap.add_argument("--broker-list", required=True, help="brokers of the cluster, CSV")
    ap.add_argument("--racks", required=True, help='{"<brokerId>": "<rack>"} JSON file or id:rack,id:rack')
    ap.add_argument("--out", default="")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--slack", type=int, default=None, help="widen the leader band by N on both sides")
    ap.add_argument("--auto-slack", action="store_true", help="use the smallest slack >= --slack that is feasible, per topic")
    ap.add_argument("--cluster", action="store_true", help="balance the leaders of all topics together: lowest cluster-wide peak, topic bands kept")
    ap.add_argument("--cluster-lo", type=int, default=None, help="with --cluster: every broker leads at least N partitions")
    ap.add_argument("--cluster-hi", type=int, default=None, help="every broker leads at most N partitions instead of the lowest peak; implies --cluster")
    ap.add_argument("--traffic", default=None, help='weigh the partitions: {"version":1,"partitions":[{"topic":..,"partition":..,"weight":N}]}')
    ap.add_argument("--sizes", default=None, help="weigh the partitions by their size: kafka-log-dirs --describe output")
    ap.add_argument("--default-weight", type=weight_arg, default=None, help="weight of the partitions the file does not name")
    ap.add_argument("--min-gain", type=u64, default=None, help="weighted: a leader moves only when it lowers its broker's lead over the target by more than N")
    ap.add_argument("--max-rounds", type=count, default=None, help="weighted: stop after N rounds")
    ap.add_argument("--exchange", action="store_true", help="weighted: when no single leader change helps, swap the leaders of two partitions on one broker pair")
    a = ap.parse_args(argv)
    weighted = a.traffic is not None or a.sizes is not None
    if a.traffic is not None and a.sizes is not None:
        ap.error("give one of --traffic and --sizes")
    if weighted and (a.slack is not None or a.auto_slack or a.cluster or a.cluster_lo is not None or a.cluster_hi is not None):
        ap.error("--traffic / --sizes cannot be combined with --slack, --auto-slack, --cluster, --cluster-lo or --cluster-hi")
    if not weighted and (a.default_weight is not None or a.min_gain is not None or a.max_rounds is not None):
        ap.error("--default-weight, --min-gain and --max-rounds need --traffic or --sizes")
    if a.exchange and not weighted:
        ap.error("--exchange needs --traffic or --sizes")
    a.slack = 0 if a.slack is None else a.slack
    a.cluster_lo = 0 if a.cluster_lo is None else a.cluster_lo
    a.cluster_hi = -1 if a.cluster_hi is None else a.cluster_hi
    if a.slack < 0:
        ap.error("--slack must be >= 0")
    cluster = a.cluster or a.cluster_hi != -1
    if a.cluster_lo < 0 or a.cluster_hi < -1:
        ap.error("--cluster-lo and --cluster-hi need a value >= 0")
    if a.cluster_lo and not cluster:
        ap.error("--cluster-lo needs --cluster")
    if cluster and a.auto_slack:
        ap.error("--auto-slack cannot be combined with --cluster")
    if cluster and a.cluster_hi >= 0 and a.cluster_hi < a.cluster_lo:
        ap.error("--cluster-hi must be >= --cluster-lo")
    rc = 0
    try:
        with open(a.current) as f:
            doc = json.load(f)
        if weighted:
            from .failover import parse_current
            fi = parse_current(doc, [int(b) for b in a.broker_list.split(",") if b], _racks(a.racks))   # input errors before the device is touched
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
            plan = _plan_weighted(fi.keys, fi.rows, fi.broker_ids, weight, a.min_gain or 0, a.max_rounds or 0, False, a.exchange)
            if a.report:
                print(weighted_report_line(plan.result), file=sys.stderr)
            text = plan_text(plan.entries)
            if a.out:
                with open(a.out, "w") as f:
                    f.write(text)
            else:
                sys.stdout.write(text)
            return 0
        if cluster:
            from .failover import parse_current
            fi = parse_current(doc, [int(b) for b in a.broker_list.split(",") if b], _racks(a.racks))   # input errors before the device is touched
            from .solver import init
            init(a.device)
            plan = _plan_cluster(fi.keys, fi.rows, fi.broker_ids, len(fi.broker_ids), a.slack, a.cluster_lo, a.cluster_hi, False)
            if plan.result.status != "OPTIMAL_PROVEN":
                print(f"kao-leaders: no choice of leaders among the replicas meets every topic's band (slack {a.slack}) and the cluster "
                      f"band ({int(plan.result.stats[7])} units unrouted); try --slack N", file=sys.stderr)
                rc = 1
            if a.report:
                print(cluster_report_line(plan.result), file=sys.stderr)
            text = plan_text(plan.entries)
            if a.out:
                with open(a.out, "w") as f:
                    f.write(text)
            else:
                sys.stdout.write(text)
            return rc
        topics = topics_from_json(doc, [int(b) for b in a.broker_list.split(",") if b], _racks(a.racks))
        for t in topics:
            bad = np.nonzero((t.current == NONE).any(axis=1))[0]
            if len(bad):
                pid = int(bad[0]) if t.partition_ids is None else int(t.partition_ids[int(bad[0])])
                raise ValueError(f"partition {t.name}-{pid} has a replica outside --broker-list or fewer replicas than its topic's "
                                 "other partitions: leader-only rebalancing keeps every replica set (use kao-cli to move replicas)")
        from .solver import init
        init(a.device)
        entries = []
        for t in topics:
            res, slack = balance_topic(t, a.slack, a.auto_slack)
            s = res.stats
            if res.status != "OPTIMAL_PROVEN":
                print(f"kao-leaders: topic {t.name}: no choice of leaders among the replicas meets the band (slack {slack}; "
                      f"{int(s[7])} units unrouted); try --slack N or --auto-slack", file=sys.stderr)
                rc = 1
            else:
                for p in np.nonzero((res.assignment != t.current).any(axis=1))[0]:
                    pid = int(p) if t.partition_ids is None else int(t.partition_ids[p])
                    entries.append((t.name, pid, [int(t.broker_ids[b]) for b in res.assignment[p]]))
            if a.report:
                print(f"topic {t.name}: status={res.status} leader_changes={res.n_changed} objective={res.objective} slack={slack} "
                      f"over_before={s[4]} under_before={s[5]} phases={s[0]} rounds={s[1]} paths={s[2]} longest_path={s[3]} "
                      f"launches={s[6]}", file=sys.stderr)
        text = plan_text(entries)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)
        else:
            sys.stdout.write(text)
    except Exception as e:  # noqa: BLE001 -- reported, exit status 1
        print(f"kao-leaders: {e}", file=sys.stderr)
        return 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
