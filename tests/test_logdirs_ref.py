"""The restatement of the log-dir balance (tests/logdirs_ref.py) against the definition's own claims, no GPU:
on the small family the bound is below the exhaustive optimum, the optimum below the peak after, the peak never rises, the end state
is move-stable and the bytes are conserved; the family is non-trivial; the result does not depend on the order of a broker's
replicas.  And the reader and the plan of kafka_assignment_optimizer_amd.logdirs: what becomes a replica, what becomes base, what is
refused, and the document of a hand-made case character for character."""
import json
import os

import numpy as np
import pytest

import logdirs_ref as lr
from conftest import GOLDEN

SEEDS = range(120)


@pytest.fixture(scope="module")
def small():
    return [(lr.small_case(s), lr.descend(**lr.small_case(s))) for s in SEEDS]


def test_small_family_bound_optimum_peak_and_stability(small):
    enumerated = at_optimum = 0
    for c, ref in small:
        assert ref["stats"][5] == 0 and lr.stable(c["dir_start"], ref["dir"], c["size"], c["base"])
        assert int(lr.loads(c["dir_start"], ref["dir"], c["size"], c["base"]).sum()) == int(lr.loads(**c).sum())
        assert [p[2] for p in ref["per_broker"]] == lr.lower_bound(**c)
        L = lr.loads(c["dir_start"], ref["dir"], c["size"], c["base"])
        for b, p in enumerate(ref["per_broker"]):
            one, mine = lr.one_broker(c, b)
            lo, hi = int(c["dir_start"][b]), int(c["dir_start"][b + 1])
            assert p[1] == int(L[lo:hi].max(initial=0)) and p[2] <= p[1] <= p[0]
            if hi == lo:
                assert p == [0] * 6
                continue
            if len(mine) == 0:
                assert p == [int(c["base"][lo:hi].max())] * 3 + [0, 0, 0]
            opt = lr.optimum(one["size"], one["base"])
            if opt is not None:
                enumerated += 1
                at_optimum += opt == p[1]
                assert p[2] <= opt <= p[1]
    print(f"brokers enumerated: {enumerated}, at their optimum: {at_optimum}")
    assert enumerated >= 120 and at_optimum >= enumerated // 2


def test_small_family_is_not_trivial(small):
    moved = sum(ref["n_moved"] > 0 for _, ref in small)
    proven = sum(ref["status"] == "OPTIMAL_PROVEN" for _, ref in small)
    print(f"moved: {moved}, on the bound: {proven}, above it: {len(small) - proven}")
    assert moved >= 60 and len(small) - proven >= 10 and proven >= 10


def test_result_does_not_depend_on_the_order_of_the_replicas():
    """The replicas permuted in the input, the r of their keys permuted with them: the same dir for every replica, the same numbers."""
    for seed in (1, 5, 10, 17, 40, 77):
        c = lr.small_case(seed)
        ref = lr.descend(**c)
        perm = np.random.default_rng(seed).permutation(len(c["dir"]))
        other = lr.descend(c["dir_start"], c["dir"][perm], c["size"][perm], c["base"], ids=perm)
        assert (other["dir"] == ref["dir"][perm]).all() and other["per_broker"] == ref["per_broker"] and other["stats"] == ref["stats"]
    c = lr.lognormal_case(2, 5, 60, 0.7, 3)
    ref = lr.descend(**c)
    perm = np.random.default_rng(0).permutation(len(c["dir"]))
    other = lr.descend(c["dir_start"], c["dir"][perm], c["size"][perm], c["base"], ids=perm)
    assert ref["n_moved"] > 0 and (other["dir"] == ref["dir"][perm]).all() and other["per_broker"] == ref["per_broker"]


def test_rounds_stops_and_crowded_counts():
    c = lr.crowded_case(3, 60)
    ref = lr.descend(**c)
    assert ref["stats"][1] == ref["stats"][2] == ref["n_moved"] == 40 and ref["peak_after"] == 100 == ref["per_broker"][0][2]   # one source: one move a round
    one = lr.descend(**c, max_rounds=1)
    assert one["stats"][:4] == [1, 1, 1, 60] and one["stats"][5] == 1 and one["n_moved"] == 1
    assert lr.descend(**c, min_gain=60 * 5)["n_moved"] == 0 and lr.descend(**c, min_gain=2 ** 64 - 1)["stats"][1] == 0
    # term (2): a base above everything else; term (0): one replica above the mean on the emptiest dir
    two = lr.descend([0, 3], [0, 0, 1], [4, 5, 6], base=[0, 0, 100])
    assert two["per_broker"][0][:3] == [100, 100, 100] and two["status"] == "OPTIMAL_PROVEN"
    zero = lr.descend([0, 3], [0, 0, 0], [50, 1, 1], base=[7, 9, 8])
    assert zero["per_broker"][0][2] == 57 and lr.bound_terms(lr.loads([0, 3], [0, 0, 0], [50, 1, 1], [7, 9, 8]), [50, 1, 1], [7, 9, 8]) == [57, 26, 9]


# ---- the reader and the plan ---------------------------------------------------------------------------------------------------------
def _doc(brokers):
    return {"version": 1, "brokers": [{"broker": b, "logDirs": [{"logDir": n, "error": err, "partitions": [
        {"partition": p, "size": s, "offsetLag": 0, "isFuture": fut} for p, s, fut in parts]} for n, err, parts in dirs]} for b, dirs in brokers]}


CURRENT = {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [1, 2]}, {"topic": "t", "partition": 1, "replicas": [2, 1]},
                                        {"topic": "a-b", "partition": 3, "replicas": [1]}, {"topic": "t", "partition": 2, "replicas": [2, 7]}]}
LOGDIRS = _doc([
    (2, [("/data/b", None, [("t-1", 10, False), ("t-2", 40, False), ("t-0", 30, False), ("gone-0", 5, False)]),
         ("/data/a", None, [("t-0", 99, True)]),
         ("/data/c", "KafkaStorageException", [("t-9", 1000, False)])]),
    (1, [("/d2", None, []), ("/d1", None, [("t-0", 50, False), ("t-1", 20, False), ("a-b-3", 60, False), ("t-2", 3, False)])]),
])


def test_reader_keeps_dirs_errors_and_future_entries():
    from kafka_assignment_optimizer_amd.logdirs import parse_log_dirs
    text = "Querying brokers for log directories information\nReceived log directory information from brokers 1,2\n" + json.dumps(LOGDIRS) + "\n"
    table = parse_log_dirs(text)
    assert table == parse_log_dirs(LOGDIRS) == parse_log_dirs(json.dumps(LOGDIRS).encode())
    assert sorted(table) == [1, 2] and list(table[2]) == ["/data/b", "/data/a", "/data/c"]
    assert table[2]["/data/c"].error == "KafkaStorageException" and table[2]["/data/b"].error is None
    assert table[2]["/data/a"].entries == [("t", 0, 99, True)] and table[1]["/d1"].entries[2] == ("a-b", 3, 60, False)
    for bad in ("no json here", json.dumps({"partitions": []}), json.dumps(_doc([(1, [("/d", None, [("nodash", 1, False)])])])),
                json.dumps(_doc([(1, [("/d", None, [("t-0", -1, False)])])])), json.dumps(_doc([(1, []), (1, [])]))):
        with pytest.raises(ValueError):
            parse_log_dirs(bad)


def test_mapping_replicas_base_and_refusals():
    from kafka_assignment_optimizer_amd.logdirs import parse_input
    li = parse_input(CURRENT, LOGDIRS)
    assert li.broker_ids == [1, 2] and li.dir_names == [["/d1", "/d2"], ["/data/a", "/data/b"]] and li.skipped == [0, 1]
    assert li.dir_start.tolist() == [0, 2, 4] and li.keys == [("a-b", 3), ("t", 0), ("t", 1), ("t", 2)]
    # replicas by (topic, partition), slots in row order: a-b-3@1, t-0@1, t-0@2, t-1@2, t-1@1, t-2@2 (broker 7 is not in the list)
    assert li.slots == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0)]
    assert li.dir.tolist() == [0, 0, 3, 3, 0, 3] and li.size.tolist() == [60, 50, 30, 10, 20, 40]
    # base: t-2 on broker 1 (not in the row), the future t-0 in /data/a, gone-0 (unknown to the current document); the failed dir counts nowhere
    assert li.base.tolist() == [3, 0, 99, 5]
    rev = parse_input(CURRENT, LOGDIRS, [2, 1])
    assert rev.broker_ids == [2, 1] and rev.dir_names == [["/data/a", "/data/b"], ["/d1", "/d2"]] and rev.base.tolist() == [99, 5, 3, 0]
    only = parse_input(CURRENT, LOGDIRS, [2, 5])   # broker 1 is left alone, broker 5 has no dir
    assert only.dir_start.tolist() == [0, 2, 2] and only.slots == [(1, 1), (2, 0), (3, 0)] and only.base.tolist() == [99, 5]
    twice = _doc([(1, [("/x", None, [("t-0", 1, False)]), ("/y", None, [("t-0", 2, False)])])])
    with pytest.raises(ValueError, match="twice"):
        parse_input(CURRENT, twice)
    parse_input(CURRENT, _doc([(1, [("/x", None, [("t-0", 1, False)]), ("/y", None, [("t-0", 2, True)])])]))   # a future copy is no duplicate
    with pytest.raises(ValueError):
        parse_input(CURRENT, LOGDIRS, [1, 1])


def test_plan_of_a_hand_made_case_is_the_expected_document(monkeypatch):
    """The library call replaced by the restatement: the plan text of the two-broker case, character for character."""
    from kafka_assignment_optimizer_amd import logdirs as ld

    def by_restatement(dir_start, dir, size, base=None, min_gain=0, max_rounds=0, dry_run=False):
        ref = lr.descend(dir_start, dir, size, base, min_gain, max_rounds)
        s = np.array([0 if x is None else x for x in ref["stats"]], dtype=np.int64)
        return ld.LogDirsResult(dir=np.asarray(dir if dry_run else ref["dir"], dtype=np.int32), n_moved=ref["n_moved"], bytes_moved=ref["bytes_moved"],
                                peak_before=ref["peak_before"], peak_after=ref["peak_after"], per_broker=np.array(ref["per_broker"], dtype=np.uint64),
                                status=ref["status"], stats=s)

    monkeypatch.setattr(ld, "balance_logdirs_arrays", by_restatement)
    plan = ld.balance_logdirs(CURRENT, LOGDIRS)
    # broker 1: /d1 = 133, /d2 = 0: a-b-3 (60) moves, then nothing gains (73 vs 60).  broker 2: /data/a = 99 (base), /data/b = 85: nothing gains
    assert plan.text() == ('{"version":1,"partitions":[\n'
                           '    {"topic":"a-b","partition":3,"replicas":[1],"log_dirs":["/d2"]}\n'
                           ']}\n')
    assert json.loads(plan.text()) == plan.document() and plan.result.n_moved == 1
    assert plan.report_lines() == [
        "logdirs: broker=1 dirs=2 skipped_dirs=0 replicas=3 peak_before=133 peak_after=73 lower_bound=67 moved=1 bytes_moved=60 rounds=1",
        "logdirs: broker=2 dirs=2 skipped_dirs=1 replicas=3 peak_before=99 peak_after=99 lower_bound=99 moved=0 bytes_moved=0 rounds=0",
        "logdirs: status=FEASIBLE_BOUND_GAP brokers=2 dirs=4 skipped_dirs=1 replicas=6 peak_before=133 peak_after=99 replicas_moved=1 bytes_moved=60 "
        "bytes_total=317 brokers_moved=1 rounds=1 moves=1 proposals=3 launches=0 stopped_by_max_rounds=0 proven=1 max_rounds_of_a_broker=1"]
    assert ld.balance_logdirs(CURRENT, LOGDIRS, dry_run=True).text() == '{"version":1,"partitions":[\n]}\n'
    wide = ld.balance_logdirs(CURRENT, LOGDIRS, min_gain=72)
    assert wide.document() == {"version": 1, "partitions": [{"topic": "a-b", "partition": 3, "replicas": [1], "log_dirs": ["/d2"]}]}
    narrow = ld.balance_logdirs(CURRENT, LOGDIRS, min_gain=112)   # only t-1 (20 bytes, slot 1 of its row) still closes such a gap: 0 + 20 + 112 < 133
    assert narrow.document() == {"version": 1, "partitions": [{"topic": "t", "partition": 1, "replicas": [2, 1], "log_dirs": ["any", "/d2"]}]}
    assert ld.balance_logdirs(CURRENT, LOGDIRS, min_gain=113).document() == {"version": 1, "partitions": []}
    # the golden file: two slots of one partition move, each inside its own broker; a future copy weighs on /disk1 as base, so a second
    # replica leaves it; a quote in a dir name is escaped
    with open(os.path.join(GOLDEN, "logdirs_two_brokers.txt")) as f:
        text = f.read()
    with open(os.path.join(GOLDEN, "logdirs_two_brokers_current.json")) as f:
        cur = json.load(f)
    plan = ld.balance_logdirs(cur, text)
    assert plan.text() == ('{"version":1,"partitions":[\n'
                           '    {"topic":"logs","partition":0,"replicas":[11,10],"log_dirs":["/mnt/\\"b\\"","/disk2"]},\n'
                           '    {"topic":"logs","partition":2,"replicas":[10,11],"log_dirs":["/disk2","any"]}\n'
                           ']}\n')
    assert json.loads(plan.text()) == plan.document()
