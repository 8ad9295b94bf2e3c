"""Hand cases of the headroom wave planner with hand-counted answers, shared by the reference's CPU tests and the GPU tests.  Every
case runs without movement caps (k = C = 0) unless it says otherwise; `want` holds wave[], n_waves, the stuck bytes and, where it
is the same in every order that can win, (least free bytes, its wave, its broker)."""
import numpy as np

N = 0xFFFF

HAND = {
    # two partitions of 60 bytes swap between two full brokers: neither fits, nothing ever leaves
    "swap": dict(cur=[[0], [1]], tgt=[[1], [0]], size=[60, 60], stored=[100, 100], capacity=[100, 100],
                 want=dict(wave=[-2, -2], n_waves=0, stuck_bytes=120, min_free=(-1, -1, -1))),
    # the same with an empty third broker at the end of the chain 0 -> 1, 1 -> 2: the 1 -> 2 move goes first and frees the room
    "chain": dict(cur=[[0], [1]], tgt=[[1], [2]], size=[60, 60], stored=[100, 100, 0], capacity=[100, 100, 100],
                  want=dict(wave=[1, 0], n_waves=2, min_free=(0, 1, 1))),
    # p: a -> b, q: c -> b, r: b -> c (a, b, c = 0, 1, 2), all 50 bytes; b has room for one arrival, c for none until q has left.
    # p first: b is full, q and r stuck.  q first: r follows into the room q frees at c, then p into the room r frees at b
    "order_decides": dict(cur=[[0], [2], [1]], tgt=[[1], [1], [2]], size=[50, 50, 50], stored=[50, 100, 100], capacity=[100, 150, 100],
                          want=dict(wave=[2, 0, 1], n_waves=3, min_free=(0, 0, 1))),
    "exact_fit": dict(cur=[[0]], tgt=[[1]], size=[40], stored=[40, 60], capacity=[100, 100],
                      want=dict(wave=[0], n_waves=1, min_free=(0, 0, 1))),
    "exact_fit_over": dict(cur=[[0]], tgt=[[1]], size=[40], stored=[40, 60], capacity=[100, 99],
                           want=dict(wave=[-2], n_waves=0, stuck_bytes=40, min_free=(-1, -1, -1))),
    # broker 1 is above its capacity: the empty partition still arrives, the 10-byte one does not
    "zero_size": dict(cur=[[0], [2]], tgt=[[1], [1]], size=[0, 10], stored=[0, 200, 10], capacity=[100, 100, 100],
                      want=dict(wave=[0, -2], n_waves=1, stuck_bytes=10, min_free=(-1, -1, -1))),
    # partition 0 only drops its replica on broker 1 (metadata-only, wave 0): its 50 bytes are free in wave 1, not in wave 0
    "metadata_removal": dict(cur=[[0, 1], [2, N]], tgt=[[0, N], [1, N]], size=[50, 50], stored=[50, 100, 50], capacity=[100, 100, 100],
                             want=dict(wave=[0, 1], n_waves=2, min_free=(0, 1, 1))),
}


def hand_case(name):
    """(cur, tgt, size, stored, capacity, C, k) of one case."""
    c = HAND[name]
    return (np.array(c["cur"], dtype=np.uint16), np.array(c["tgt"], dtype=np.uint16), np.array(c["size"], dtype=np.uint64),
            list(c["stored"]), list(c["capacity"]), c.get("C", 0), c.get("k", 0))
