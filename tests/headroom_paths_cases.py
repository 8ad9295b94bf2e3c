"""Instances shared by tests/test_waves_headroom_paths_ref.py (CPU) and tests/test_gpu_waves_headroom_paths.py (MI355X): one
case per kernel path of kao_plan_waves_headroom at its smallest shape.  Capacities above 2^63, broker indices beyond one
workgroup's 256 threads, ties of the least free bytes within a thread, between threads and between waves, the row shapes and
the mid-size plan of waves_paths_cases under scaled capacities, and plans whose last order ends on either side of the host's
check after 32 rounds.  A case is (name, cur, tgt, size, stored, capacity, C, k, seed)."""
import numpy as np

import waves_headroom_ref as hr
import waves_paths_cases as wc

U64_MAX = (1 << 64) - 1
CAP40 = 1 << 40


def _rows(moves):
    """Width-1 rows of (source, target) pairs."""
    return (np.array([[s] for s, _ in moves], dtype=np.uint16), np.array([[t] for _, t in moves], dtype=np.uint16))


def _case(name, moves, size, B, capacity, k=0, extra=None, seed=1):
    """Width 1, C = 0: stored = what the rows hold plus `extra` {broker: bytes}; capacity = a value for every broker or
    ({broker: bytes}, the value of the others)."""
    cur, tgt = _rows(moves)
    size = np.array(size, dtype=np.uint64)
    stored = hr.stored_from_rows(cur, size, B)
    for b, v in (extra or {}).items():
        stored[b] += v
    if isinstance(capacity, tuple):
        capacity = [capacity[0].get(b, capacity[1]) for b in range(B)]
    else:
        capacity = [capacity] * B
    return (name, cur, tgt, size, stored, capacity, 0, k, seed)


# ---- capacities above 2^63: every free value is clamped to 2^63 - 1 before it is compared ----

def clamp_cases():
    """clamp/all: brokers 1 and 2 receive bytes in wave 0 and both have more than 2^63 - 1 bytes free, so the clamped values tie
    and the lowest broker, 1, is reported; unclamped, broker 2 has fewer (2^64 - 1 - 100 - 15 against 2^64 - 1 - 0 - 10).
    clamp/control: the same rows at capacity 2^63, where nothing is clamped and broker 2 is the strict minimum.
    clamp/waves: two partitions of equal size share their source at k = 1, so order 0 (ties by partition index) sends partition 0
    to broker 1 in wave 0 and partition 1 to broker 2 in wave 1; both free values are clamped and wave 0 keeps the tie, although
    broker 2 holds 100 bytes more."""
    moves, size, stored = [(0, 1), (0, 2), (3, 2)], [10, 10, 5], [20, 0, 100, 5]
    out = []
    for name, cap in (("clamp/all", U64_MAX), ("clamp/control", hr.UNLIMITED)):
        c = _case(name, moves, size, 4, cap)
        out.append(c[:4] + (list(stored),) + c[5:])
    c = _case("clamp/waves", [(0, 1), (0, 2)], [10, 10], 3, U64_MAX, k=1)
    out.append(c[:4] + ([20, 0, 100],) + c[5:])
    return out


# ---- broker indices beyond 256 x (workgroups per order) ----

WIDE_MOVES = [(10, 999), (300, 999), (600, 999), (998, 999), (5, 700)]
WIDE_TO_257 = {10: 10, 300: 100, 600: 200, 998: 255, 5: 5, 999: 256, 700: 250}


def wide_cases():
    """Five moving partitions (one workgroup per order) on 1,000 brokers: four of them arrive at broker 999 at k = 1, one per
    wave, so the minimum key bid at broker 999 has to be cleared between rounds by a thread whose index is far below 999.  The
    same rows over 257 brokers, with broker 256 in the role of 999: one past the workgroup."""
    return [_case("wide/1000", WIDE_MOVES, [7] * 5, 1000, CAP40, k=1),
            _case("wide/257", [(WIDE_TO_257[s], WIDE_TO_257[t]) for s, t in WIDE_MOVES], [7] * 5, 257, CAP40, k=1)]


# ---- ties of the least free bytes: k_head_close walks the brokers 256 apart per thread, reduces over the threads, and keeps
# ---- the running minimum over the waves ----

def tie_cases():
    """1,000 brokers, sizes 10; the named targets hold 50 bytes more and have capacity 100, so each has 40 bytes free after its
    arrival (39 at broker 999 of tie/strict).
    tie/thread: brokers 44 and 300 = 44 + 256 fall to one thread, which has to keep the first.
    tie/threads: brokers 45 and 700 fall to threads 45 and 188; the reduction has to prefer the lower broker.
    tie/strict: the strict minimum sits at broker 999, the last stride of thread 231.
    tie/waves: both partitions leave broker 0 at k = 1, so partition 0 (to broker 44) takes wave 0 and partition 1 (to broker 3)
    wave 1; the earlier wave keeps the tie although broker 3 is lower."""
    def tie(name, moves, extra, k=0):
        return _case(name, moves, [10] * len(moves), 1000, ({b: 100 for b in extra}, CAP40), k=k, extra=extra)
    return [tie("tie/thread", [(0, 300), (1, 44)], {300: 50, 44: 50}),
            tie("tie/threads", [(0, 700), (1, 45)], {700: 50, 45: 50}),
            tie("tie/strict", [(0, 999), (1, 45), (2, 300)], {999: 51, 45: 50, 300: 50}),
            tie("tie/waves", [(0, 44), (0, 3)], {44: 50, 3: 50}, k=1)]


# ---- the row shapes and the mid-size plan of waves_paths_cases, under capacities scaled from the rows ----

SHAPE_FACTORS = (100, 110, 120)


def _scaled(case, factor):
    name, cur, tgt, size, C, k, seed = case
    stored, capacity = hr.scaled_capacity(cur, tgt, size, wc.brokers_of(case), factor)
    return (f"{name}@{factor}", cur, tgt, size, stored, capacity, C, k, seed)


def sized_shape_cases():
    """The sized cases of wc.shape_cases() (byte cap alone, both caps)."""
    return [c for c in wc.shape_cases() if c[0].endswith(("/C0", "/C2"))]


def shape_cases():
    return [_scaled(c, f) for c in sized_shape_cases() for f in SHAPE_FACTORS]


SHAPE_NAMES = tuple(f"{c[0]}@{f}" for c in sized_shape_cases() for f in SHAPE_FACTORS)

# name -> capacity factor: 1,000 moving partitions on 40 brokers, four workgroups per order
MID = {"loguniform/C2": 100, "equal/C0": 100, "oversized/C2": 102, "zeros/02": 102}


def mid_case(name):
    return _scaled(wc.mid_case(name), MID[name])


# ---- the host loop's check after every 32 rounds ----

def conveyor(n, fork=False):
    """Partition i moves 10 bytes from broker i to broker i + 1 (i < n); every broker's capacity is what it holds, and broker n
    holds nothing.  Partition n - 1 fits in wave 0; partition i < n - 1 fits only in the wave after partition i + 1 has left
    broker i + 1, because departures free room for later waves only.  So every order takes partition n - 1 - w in wave w: n waves.

    Rounds, k = C = 0: in the first round of a wave every undecided partition tests the fit; the one that
    fits finds no bid of the previous round at its brokers and bids, the others skip the wave.  In the second round it holds the
    minimum at its target and at its source and joins; nobody bids, so the close step ends the wave.  Two rounds per wave: wave
    w takes rounds 2w and 2w + 1.  After wave n - 1 nothing is undecided: round 2n has neither a bidder nor a joiner and no
    departure is pending, so the order is done in round index 2n.

    With `fork`, broker n holds two partitions of 10 bytes that move to the empty brokers n + 1 and n + 2.  Both fit in wave 0
    and both bid at their shared source in round 0; in round 1 the lower key holds the minimum at both of its brokers and joins,
    the other sees the first one's key at the source and bids again; in round 2 it joins.  Wave 0 takes three rounds, partition
    n - 1 - (w - 1) follows in wave w >= 1 at rounds 2w + 1 and 2w + 2, and the order is done in round index 2n + 3: n + 1 waves
    over n + 2 partitions.

    The host reads the count of finished orders after every 32 rounds, so stats[4] is 32 when that index is at most 31 and 64
    when it is 32."""
    moves = [(i, i + 1) for i in range(n)] + ([(n, n + 1), (n, n + 2)] if fork else [])
    B = n + 3 if fork else n + 1
    cur, tgt = _rows(moves)
    size = np.full(len(moves), 10, dtype=np.uint64)
    stored = hr.stored_from_rows(cur, size, B)
    capacity = [max(s, 10) for s in stored]
    return (f"conveyor/{n}{'+fork' if fork else ''}", cur, tgt, size, stored, capacity, 0, 0, 1)


def conveyor_cases():
    """(case, index of the round in which every order is done, stats[4]).  15 waves: round 30.  14 waves after a three-round
    wave: round 31, the last of the first batch.  16 waves: round 32, the first of the second batch."""
    return [(conveyor(15), 30, 32), (conveyor(14, fork=True), 31, 32), (conveyor(16), 32, 64)]


def all_cases():
    return (clamp_cases() + wide_cases() + tie_cases() + shape_cases() + [mid_case(n) for n in MID]
            + [c for c, _, _ in conveyor_cases()])
