"""Fast restatement of kao_oracle.canonicalize, and the inputs the canonical tie-break is tested on.

kao_oracle.canonicalize verifies the whole assignment for every trial move (92 s at 140 brokers x 130 partitions).  canon_ref
follows the same definition -- scanning partitions and slots in order, every newly placed replica moves to the lowest broker
index that keeps the candidate feasible with the same objective, repeated to a fixpoint, then the follower order -- but keeps the
counts the rows of the model are made of (replicas and leaders per broker, replicas per rack and per partition per rack) and
tests all lower indices of one replica in one vectorised step.  In a feasible state a move keeps every row satisfied iff the few
counts it changes stay inside their bands, which is what the mask below asks.  tests/test_canon_ref.py holds it against
kao_oracle.canonicalize bit for bit; tests/test_gpu_canon.py holds k_canon against it.
"""
import numpy as np

NONE = 0xFFFF

# (B0, R, P, rf, removed, added, new_rf): small enough for kao_oracle.canonicalize
SMALL_SHAPES = [
    (24, 3, 40, 3, [], [(24, 0), (25, 1), (26, 2)], None),
    (30, 5, 36, 6, [3, 7], [(30, 3), (31, 2)], None),
    (28, 4, 30, 4, [5], [(28, 1)], 5),
    (28, 4, 44, 5, [5, 6], [(28, 1), (29, 2)], 3),
    (20, 1, 70, 2, [1], [(20, 0), (21, 0)], None),
    (16, 2, 33, 1, [2], [(16, 0)], None),
]
SMALL_CASES = [(i, slack) for i in range(len(SMALL_SHAPES)) for slack in (False, True)]


def canon_ref(topic, assign):
    """-> (canonical assignment [P, RF] uint16, passes, moves): passes counts the scans of the fixpoint loop (the last one moves
    nothing), moves the accepted moves.  An infeasible input is returned as it is, with (0, 0)."""
    import kao_oracle as ko
    P, RF, B, R = topic.n_partitions, topic.rf, topic.n_brokers, topic.n_racks
    a = np.asarray(assign).reshape(P, RF).astype(np.int64).copy()
    if ko.verify(topic, a)[1][0] != 0:
        return a.astype(np.uint16), 0, 0
    bd = topic.bounds()
    rack = np.asarray(topic.rack_of, dtype=np.int64)
    cnt_r = np.bincount(a.ravel(), minlength=B)
    cnt_l = np.bincount(a[:, 0], minlength=B)
    rack_cnt = np.bincount(rack[a.ravel()], minlength=R)
    prack = np.zeros((P, R), dtype=np.int64)
    np.add.at(prack, (np.repeat(np.arange(P), RF), rack[a.ravel()]), 1)
    # objective coefficient of broker b in a slot where it is not a current replica of the partition (leader slot, follower slot)
    bw = np.zeros(B, dtype=np.int64) if topic.broker_w is None else np.asarray(topic.broker_w, dtype=np.int64)
    bwl = np.zeros(B, dtype=np.int64) if topic.broker_wl is None else np.asarray(topic.broker_wl, dtype=np.int64)
    coef = (bw + bwl, bw)
    in_cur = np.zeros((P, B), dtype=bool)
    for p in range(P):
        for v in topic.current[p]:
            if int(v) != NONE and int(v) < B:
                in_cur[p, int(v)] = True
    passes = moves = 0
    changed = True
    while changed:
        changed = False
        passes += 1
        for p in range(P):
            for k in range(RF):
                b = int(a[p, k])
                if in_cur[p, b] or b == 0:
                    continue
                rb = int(rack[b])
                rn = rack[:b]
                ok = ~in_cur[p, :b]
                ok[a[p][a[p] < b]] = False
                ok &= coef[0 if k == 0 else 1][:b] == coef[0 if k == 0 else 1][b]
                ok &= cnt_r[:b] + 1 <= bd["rep_hi"]
                leave = cnt_r[b] - 1 >= bd["rep_lo"]
                if k == 0:
                    ok &= cnt_l[:b] + 1 <= bd["lead_hi"]
                    leave = leave and cnt_l[b] - 1 >= bd["lead_lo"]
                other = rn != rb
                rack_ok = (rack_cnt[rn] + 1 <= bd["rack_hi"]) & (prack[p, rn] + 1 <= bd["prack_hi"])
                if not (rack_cnt[rb] - 1 >= bd["rack_lo"] and prack[p, rb] - 1 >= bd["prack_lo"]):
                    rack_ok[:] = False
                ok &= ~other | rack_ok
                if not leave or not ok.any():
                    continue
                nb = int(np.argmax(ok))
                a[p, k] = nb
                cnt_r[b] -= 1; cnt_r[nb] += 1
                if k == 0:
                    cnt_l[b] -= 1; cnt_l[nb] += 1
                rack_cnt[rb] -= 1; rack_cnt[rack[nb]] += 1
                prack[p, rb] -= 1; prack[p, rack[nb]] += 1
                changed = True
                moves += 1
    for p in range(P):
        cur = [int(v) for v in topic.current[p] if int(v) != NONE]
        fol = [int(v) for v in a[p, 1:]]
        kept = [b for b in cur if b in fol]
        new = sorted(b for b in fol if b not in kept)
        a[p, 1:] = kept + new
    return a.astype(np.uint16), passes, moves


def slack_override(topic):
    """The derived bands widened: rep_hi + 1, lead_hi + 1, rack_hi + 2, rack_lo - 2 (not below 0)."""
    bd = topic.bounds()
    return {"rep_hi": bd["rep_hi"] + 1, "lead_hi": bd["lead_hi"] + 1, "rack_hi": bd["rack_hi"] + 2, "rack_lo": max(bd["rack_lo"] - 2, 0)}


def canon_input(shape, slack=False, rack_of=None):
    """-> (oracle Topic, feasible assignment [P, RF] uint16) built without a solver: the cluster of `shape` after its brokers left
    and joined, a balanced fill of the target brokers (the first rotation of (1, 2, 3, 5, 7) that is feasible), and then the
    brokers permuted inside every rack -- which keeps every count of the model and makes most replicas new.  `rack_of` replaces
    the rack map (b mod R) of the target brokers."""
    import kao_oracle as ko
    B0, R, P, rf, removed, added, new_rf = shape
    ot = ko.make_cluster("canon", B0, R, 1, P, rf, removed, added, new_rf=new_rf).topics[0]
    if rack_of is not None:
        ot.rack_of = np.asarray(rack_of, dtype=np.uint8)
    if slack:
        ot.bounds_override = slack_override(ot)
    B = ot.n_brokers
    a0 = None
    for t in (1, 2, 3, 5, 7):
        a0 = ko.balanced_fill(B, R, P, ot.rf, t, [int(r) for r in ot.rack_of])
        if ko.verify(ot, a0)[1][0] == 0:
            break
    else:
        raise ValueError(f"no feasible balanced fill for {shape} (slack={slack})")
    rng = np.random.default_rng(7)
    pi = np.arange(B)
    for r in range(R):
        members = np.flatnonzero(np.asarray(ot.rack_of) == r)
        pi[members] = rng.permutation(members)
    return ot, pi[a0.astype(np.int64)].astype(np.uint16)


def new_fraction(topic, assign):
    """Share of the replicas of `assign` that are not current replicas of their partition."""
    a = np.asarray(assign).reshape(topic.n_partitions, topic.rf)
    n = sum(1 for p in range(topic.n_partitions) for b in a[p] if int(b) not in {int(v) for v in topic.current[p]})
    return n / a.size
