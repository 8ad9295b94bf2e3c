"""Fast, deterministic builder of huge topics (10^6 replica slots and more) for the GPU tests of tests/test_gpu_huge.py.

kao_oracle.make_cluster / synthetic.make_cluster place replicas one at a time (seconds at 400,000 partitions); this builder places
them with numpy in a fraction of a second.  The old cluster has brokers 0..B0-1, broker b in rack b mod R (R divides B0).  Slot k of
partition p goes to old broker (p + k * step) mod B0 with step = 1 (mod R): the slots of a partition land on racks p, p + 1, ...
(round robin), the rows are distinct, and every column is a cyclic shift of the brokers, so replicas and leaders are balanced.
`removed` brokers leave (their slots become holes), `added` (id, rack) brokers join; the target broker list is the survivors
ascending, then the added ones, as in make_cluster.  `new_rf` changes the replication factor; `drift` moves that fraction of each
column's slots to a random target broker not already in the row (seeded)."""
import numpy as np

NONE = 0xFFFF


def huge_topic(B0, R, P, rf, removed=(), added=(), new_rf=None, drift=0.0, seed=1, bounds_override=None, name="huge"):
    """-> (oracle Topic, product Topic) of one topic."""
    import kao_oracle as ko
    from conftest import to_product_topic
    assert B0 % R == 0 and B0 >= rf * R, (B0, R, rf)
    q = B0 // (rf * R)
    step = R * q + 1                                     # (rf - 1) * step < B0: the rf slots of a row are distinct brokers
    old = (np.arange(P, dtype=np.int64)[:, None] + np.arange(rf, dtype=np.int64)[None, :] * step) % B0
    gone = np.zeros(B0, dtype=bool)
    gone[np.asarray(list(removed), dtype=np.int64)] = True
    survivors = np.flatnonzero(~gone)
    target = np.concatenate([survivors, np.asarray([b for b, _ in added], dtype=np.int64)])
    rack = np.concatenate([survivors % R, np.asarray([r for _, r in added], dtype=np.int64)]).astype(np.uint8)
    lut = np.full(B0, NONE, dtype=np.uint16)
    lut[survivors] = np.arange(len(survivors), dtype=np.uint16)
    cur = lut[old]
    if drift > 0:
        rng = np.random.default_rng(seed)
        B = len(target)
        for k in range(rf):                              # one column at a time: a partition is touched at most once per pass
            idx = np.flatnonzero(rng.random(P) < drift)
            nb = rng.integers(0, B, len(idx)).astype(np.uint16)
            ok = ~(cur[idx] == nb[:, None]).any(axis=1)
            cur[idx[ok], k] = nb[ok]
    ot = ko.Topic(name=name, broker_ids=target.astype(np.int32), rack_of=rack, n_racks=R, n_partitions=P, rf=new_rf or rf,
                  current=np.ascontiguousarray(cur), bounds_override=dict(bounds_override or {}))
    return ot, to_product_topic(ot)


def check_validate_limits(ot):
    """The limits kao_model.cpp::validate puts on a topic: <= 4,000,000 slots, <= 65,535 current replicas on a broker, an average of
    <= 30,000 replicas per broker."""
    n = ot.n_partitions * ot.rf
    cnt = np.bincount(ot.current[ot.current != NONE].astype(np.int64), minlength=ot.n_brokers)
    assert n <= 4_000_000 and cnt.max() <= 65535 and -(-n // ot.n_brokers) <= 30000, (n, int(cnt.max()), ot.n_brokers)
