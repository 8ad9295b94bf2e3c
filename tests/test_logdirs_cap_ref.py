"""The restatement of the log-dir planners by utilisation (tests/logdirs_cap_ref.py) against the definition, on
the CPU: 120 seeded instances.  The restatement itself asserts, round by round, that the peak utilisation never rises, that the sorted
utilisations fall and that winners share no dir; here: the end state is move-stable by brute force, placed replicas are stable without
rounds, bound <= optimum <= peak wherever the optimum can be enumerated, proven implies optimal (which is what validates the
integrality test), the identities with the byte planners at equal capacities, and independence from the order of the arrays."""
import numpy as np
import pytest

import logdirs_cap_ref as cr
import logdirs_ref as lr
import place_ref as pr

SEEDS = range(120)
EQUAL = (1, 12345, None)   # None: 2^61 / n_dirs


def _equal_caps(value, D):
    return np.full(D, (2 ** 61 // max(D, 1)) if value is None else value, dtype=np.int64)


@pytest.fixture(scope="module")
def balanced():
    out = []
    for seed in SEEDS:
        c = cr.small_case_cap(seed)
        trace = {}
        out.append((c, cr.descend(c["dir_start"], c["dir"], c["size"], c["cap"], c["base"], trace=trace), trace))
    return out


@pytest.fixture(scope="module")
def placed():
    out = []
    for seed in SEEDS:
        c = cr.small_place_case_cap(seed)
        out.append((c, {m: cr.place(c["dir_start"], c["broker"], c["dir"], c["size"], c["cap"], c["base"], m) for m in (False, True)}))
    return out


def test_the_family_exercises_the_walk_the_test_and_the_gap(balanced):
    """Conditions the restatement meets by itself: enough seeds propose a dir that is neither c1 nor the last in rank, end with the
    integrality test alone, and end with a gap."""
    walk = sum(t.get("walk", 0) > 0 for _, _, t in balanced)
    test_only = sum(any(p[9] == 2 for p in ref["per_broker"]) for _, ref, _ in balanced)
    gap = sum(any(p[9] == 0 for p in ref["per_broker"]) for _, ref, _ in balanced)
    print(f"seeds with a walk proposal: {walk}, with proof 2: {test_only}, with a gap: {gap}")
    assert walk >= 10 and test_only >= 10 and gap >= 10


def test_end_state_is_move_stable_and_conserves_bytes(balanced):
    for c, ref, _ in balanced:
        assert cr.stable_cap(c["dir_start"], ref["dir"], c["size"], c["cap"], c["base"])
        assert sum(cr.loads(c["dir_start"], ref["dir"], c["size"], c["base"])) == sum(cr.loads(c["dir_start"], c["dir"], c["size"], c["base"]))
        bod = lr.broker_of_dir(c["dir_start"])
        assert (bod[ref["dir"]] == bod[c["dir"]]).all() if len(c["dir"]) else True
        for p in ref["per_broker"]:
            assert not cr.above(p[2], p[3], p[0], p[1])       # the peak never rises
            assert not cr.above(p[4], p[5], p[2], p[3])       # bound <= peak


def test_min_gain_and_max_rounds(balanced):
    for seed in range(0, 120, 7):
        c = balanced[seed][0]
        for mg in (1, 25, 2 ** 64 - 1):
            ref = cr.descend(c["dir_start"], c["dir"], c["size"], c["cap"], c["base"], min_gain=mg)
            assert cr.stable_cap(c["dir_start"], ref["dir"], c["size"], c["cap"], c["base"], mg)
            assert mg < 2 ** 64 - 1 or ref["n_moved"] == 0
        one = cr.descend(c["dir_start"], c["dir"], c["size"], c["cap"], c["base"], max_rounds=1)
        assert one["stats"][7] <= 1 and one["stats"][5] == sum(p[8] > 1 for p in balanced[seed][1]["per_broker"])


def test_bound_optimum_peak_and_proofs(balanced):
    """bound <= optimum <= peak, and a proven broker is at its optimum: by the bound or by the integrality test alone."""
    enumerated = by_test = 0
    for c, ref, _ in balanced:
        for b, p in enumerate(ref["per_broker"]):
            sub, _ = cr.one_broker(c, b)
            if not len(sub["base"]):
                continue
            opt = cr.optimum_cap(sub["size"], [int(x) for x in sub["base"]], [int(x) for x in sub["cap"]])
            if opt is None:
                continue
            enumerated += 1
            assert not cr.above(p[4], p[5], *opt) and not cr.above(*opt, p[2], p[3])
            if p[9]:
                assert opt[0] * p[3] == p[2] * opt[1]
                by_test += p[9] == 2
    print(f"brokers enumerated: {enumerated}, proven by the integrality test alone: {by_test}")
    assert enumerated >= 150 and by_test >= 10   # most brokers of the family are small enough to enumerate


def test_place_bound_optimum_peak_and_proofs(placed):
    enumerated = 0
    for c, refs in placed:
        ds = [int(x) for x in c["dir_start"]]
        for move, ref in refs.items():
            for b, p in enumerate(ref["per_broker"]):
                sub, _ = cr.one_place_broker(c, b)
                n = len(sub["base"])
                if not n:
                    continue
                res = sub["dir"] >= 0
                fixed = [int(x) for x in sub["base"]]
                if not move:
                    for x, w in zip(sub["dir"][res], sub["size"][res]):
                        fixed[int(x)] += int(w)
                opt = cr.optimum_cap(sub["size"] if move else sub["size"][~res], fixed, [int(x) for x in sub["cap"]])
                if opt is None:
                    continue
                enumerated += 1
                assert not cr.above(p[4], p[5], *opt) and not cr.above(*opt, p[2], p[3])
                if p[11]:
                    assert opt[0] * p[3] == p[2] * opt[1]
            assert ds[-1] == len(c["cap"])
    assert enumerated >= 300


def test_placed_replicas_are_stable_without_rounds(placed):
    for c, refs in placed:
        ref = refs[False]
        home = [r for r in range(len(c["dir"])) if c["dir"][r] < 0]
        assert cr.stable_cap(c["dir_start"], ref["dir"], c["size"], c["cap"], c["base"], only=home)
        assert (ref["dir"][c["dir"] >= 0] == c["dir"][c["dir"] >= 0]).all() and (ref["dir"] >= 0).all()
        assert cr.stable_cap(c["dir_start"], refs[True]["dir"], c["size"], c["cap"], c["base"])


@pytest.mark.parametrize("value", EQUAL)
def test_equal_capacities_give_the_byte_planner(value):
    """dir[], the counters, the bytes of the peaks, status, and the L, moved, bytes, placed and rounds columns; every stats entry."""
    for seed in SEEDS:
        c = lr.small_case(seed)
        cap = _equal_caps(value, int(c["dir_start"][-1]))
        ref, byt = cr.descend(c["dir_start"], c["dir"], c["size"], cap, c["base"]), lr.descend(c["dir_start"], c["dir"], c["size"], c["base"])
        assert ref["dir"].tobytes() == byt["dir"].tobytes() and ref["status"] == byt["status"] and ref["stats"] == byt["stats"]
        assert (ref["n_moved"], ref["bytes_moved"], ref["peak_before"][0], ref["peak_after"][0]) == (byt["n_moved"], byt["bytes_moved"], byt["peak_before"], byt["peak_after"])
        assert [[p[0], p[2], p[6], p[7], p[8]] for p in ref["per_broker"]] == [[q[0], q[1], q[3], q[4], q[5]] for q in byt["per_broker"]]
        assert all((p[9] > 0) == (q[1] == q[2]) for p, q in zip(ref["per_broker"], byt["per_broker"]))
        c = pr.small_case(seed)
        for move in (False, True):
            ref = cr.place(c["dir_start"], c["broker"], c["dir"], c["size"], cap, c["base"], move)
            byt = pr.place(c["dir_start"], c["broker"], c["dir"], c["size"], c["base"], move)
            assert ref["dir"].tobytes() == byt["dir"].tobytes() and ref["status"] == byt["status"] and ref["stats"] == byt["stats"]
            assert [ref[k] for k in ("n_placed", "bytes_placed", "n_moved", "bytes_moved")] == [byt[k] for k in ("n_placed", "bytes_placed", "n_moved", "bytes_moved")]
            assert (ref["peak_before"][0], ref["peak_after"][0]) == (byt["peak_before"], byt["peak_after"])
            assert [[p[0], p[2]] + p[6:11] for p in ref["per_broker"]] == [[q[0], q[1]] + q[3:8] for q in byt["per_broker"]]


def test_place_without_homeless_is_the_balance_call(balanced):
    for c, ref, _ in balanced:
        broker = lr.broker_of_dir(c["dir_start"])[c["dir"]] if len(c["dir"]) else np.zeros(0, dtype=np.int64)
        got = cr.place(c["dir_start"], broker, c["dir"], c["size"], c["cap"], c["base"], True)
        assert got["dir"].tobytes() == ref["dir"].tobytes() and got["status"] == ref["status"] and got["peak_before"] == ref["peak_before"]
        assert [p[:6] + p[8:] for p in got["per_broker"]] == ref["per_broker"] and got["n_placed"] == 0
        still = cr.place(c["dir_start"], broker, c["dir"], c["size"], c["cap"], c["base"], False)
        assert still["dir"].tobytes() == np.asarray(c["dir"], dtype=np.int64).tobytes() and still["status"] == "OPTIMAL_PROVEN"


def test_result_does_not_depend_on_the_order_of_the_arrays(balanced, placed):
    """The replicas permuted, their r kept in ids: the same dirs replica by replica, the same rows."""
    for seed in range(0, 120, 3):
        c, ref, _ = balanced[seed]
        perm = np.random.default_rng(500 + seed).permutation(len(c["dir"]))
        got = cr.descend(c["dir_start"], c["dir"][perm], c["size"][perm], c["cap"], c["base"], ids=perm)
        assert got["dir"].tobytes() == ref["dir"][perm].tobytes() and got["per_broker"] == ref["per_broker"]
        c, refs = placed[seed]
        for move in (False, True):
            got = cr.place(c["dir_start"], c["broker"][perm], c["dir"][perm], c["size"][perm], c["cap"], c["base"], move, ids=perm)
            assert got["dir"].tobytes() == refs[move]["dir"][perm].tobytes() and got["per_broker"] == refs[move]["per_broker"]
