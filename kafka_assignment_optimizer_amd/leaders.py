"""Leader-only rebalancing: the fewest preferred-leader changes that put every broker inside the leader band, replica sets kept
(kao_balance_leaders).

    python -m kafka_assignment_optimizer_amd.leaders --current current.json --broker-list 0,1,2 --racks racks.json --out plan.json

writes a reassignment document that holds only the partitions whose preferred leader changes; every row is the current row with
the new leader swapped to the front, so `kafka-reassign-partitions --execute` moves no data (kao-waves puts the whole plan in one
wave).  Topics are balanced one by one: the band is floor / ceil of partitions / brokers per topic, `--slack N` widens it by N on
both sides, `--auto-slack` takes the smallest N that is feasible.  The answer is exact: n_changed is the proven minimum, or the
topic is proven infeasible (no choice of leaders among its replicas meets the band).
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _ffi
from .model import NONE, Topic, topics_from_json
from .solver import STATUS_NAMES, _check, _CTopics

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


def plan_text(entries) -> str:
    """The reassignment document of [(topic, partition, replicas)], byte for byte as cli/kao-leaders writes it."""
    rows = ['    {"topic":"%s","partition":%d,"replicas":[%s]}' % (t.replace("\\", "\\\\").replace('"', '\\"'), p, ",".join(str(b) for b in r))
            for t, p, r in entries]
    return '{"version":1,"partitions":[' + "".join(("\n" if i == 0 else ",\n") + r for i, r in enumerate(rows)) + "\n]}\n"


def _racks(arg: str) -> dict:
    if ":" in arg and "{" not in arg and not arg.endswith(".json"):
        return {int(k): v for k, v in (kv.split(":") for kv in arg.split(",") if kv)}
    with open(arg) as f:
        return {int(k): str(v) for k, v in json.load(f).items()}


def main(argv=None) -> int:
    """Python twin of cli/kao-leaders: same flags, same bytes, same exit status (0 ok, 1 error or infeasible, 2 usage)."""
    ap = argparse.ArgumentParser(prog="kao-leaders", description="fewest preferred-leader changes that balance the leaders; moves no data")
    ap.add_argument("--current", required=True, help="reassignment JSON of the cluster as it is")
    ap.add_argument("--broker-list", required=True, help="brokers of the cluster, CSV")
    ap.add_argument("--racks", required=True, help='{"<brokerId>": "<rack>"} JSON file or id:rack,id:rack')
    ap.add_argument("--out", default="")
    ap.add_argument("--report", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--slack", type=int, default=0, help="widen the leader band by N on both sides")
    ap.add_argument("--auto-slack", action="store_true", help="use the smallest slack >= --slack that is feasible, per topic")
    a = ap.parse_args(argv)
    if a.slack < 0:
        ap.error("--slack must be >= 0")
    rc = 0
    try:
        with open(a.current) as f:
            doc = json.load(f)
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
