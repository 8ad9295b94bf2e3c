"""Instances shared by tests/test_waves_cap_ref.py (CPU) and tests/test_gpu_waves_paths.py (MI355X): the family on which the
wave cap is checked and found tight, the plans whose winning order comes late (order budget), stars, a mid-size plan and the
row shapes.  A case is (name, cur, tgt, size, C, k, seed); size None = the count-only planner (C unused)."""
import functools

import numpy as np

import waves_ref as wr
import waves_sized_ref as sr

NONE = wr.NONE
GIB = 1 << 30


def run_model(case, n_orders=64, with_winner=False):
    _, cur, tgt, size, C, k, seed = case
    if size is None:
        return wr.kernel_model(cur, tgt, k, seed, n_orders, with_winner)
    return sr.kernel_model_sized(cur, tgt, size, C, k, seed, n_orders, with_winner)


def case_cap(case):
    _, cur, tgt, size, C, k, _ = case
    return wr.wave_cap(cur, tgt, k) if size is None else sr.wave_cap_sized(cur, tgt, size, C, k)


def case_fits(case, n_orders=64):
    _, cur, tgt, size, C, k, seed = case
    return wr.order_fits(cur, tgt, k, seed, n_orders) if size is None else sr.order_fits_sized(cur, tgt, size, C, k, seed, n_orders)


def n_moving(case):
    return sum(1 for s in wr.classify(case[1], case[2])[1] if s)


@functools.lru_cache(maxsize=None)
def cap_family():
    """240 small plans (at most 16 changed partitions each): the generators of the two reference modules as they are, and the
    same rows with all sizes equal, with C = 1, with sizes in 0..3 under C in 1..5, and without a count cap."""
    fam = []
    for s in range(40):
        cur, tgt, k = wr.random_instance(s, 16)
        fam.append((f"count-{s}", cur, tgt, None, 0, k, s + 1))
        P = cur.shape[0]
        rng = np.random.default_rng(7000 + s)
        fam.append((f"equal-{s}", cur, tgt, np.full(P, GIB, dtype=np.uint64), GIB * int(rng.integers(1, 4)), k if s % 2 else 0, s + 1))
        fam.append((f"tiny-{s}", cur, tgt, rng.integers(0, 4, P).astype(np.uint64), int(rng.integers(1, 6)), k if s % 2 else 0, s + 1))
        fam.append((f"tinyk-{s}", cur, tgt, rng.integers(0, 4, P).astype(np.uint64), int(rng.integers(1, 6)), 0, s + 1))
        scur, stgt, size, C, sk = sr.random_sized_instance(s, 16)
        fam.append((f"sized-{s}", scur, stgt, size, C, sk, s + 1))
        fam.append((f"c1-{s}", scur, stgt, size, 1, sk, s + 1))
    return fam


# cap_family() indices of the plans where some order's first fit uses exactly wave_cap waves, and how many of the 240 x 64 first
# fits do (found on the CPU, verified by tests/test_waves_cap_ref.py)
TIGHT = (98, 102, 129, 138, 139, 162, 163, 169, 234, 235, 236, 237, 238)
TIGHT_FITS = 801


def scaled_instance(seed, P, B, rf):
    """wr.random_instance's generator at a chosen size: P partitions of RF rf on B brokers, 5 % leader changes, 90 % moving."""
    rng = np.random.default_rng(seed)
    cur = np.array([rng.choice(B, rf, replace=False) for _ in range(P)], dtype=np.uint16)
    tgt = cur.copy()
    for p in range(P):
        r = rng.random()
        if r < 0.05:
            tgt[p] = np.roll(cur[p], 1)
        elif r < 0.95:
            n_new = int(rng.integers(1, rf + 1))
            free = [b for b in range(B) if b not in cur[p]]
            slots = rng.choice(rf, min(n_new, len(free)), replace=False)
            tgt[p, slots] = rng.choice(free, len(slots), replace=False)
    return cur, tgt


def tied_sizes(n, seed):
    """1, 2 or 3 GiB each: three traffic codes at the added brokers, so the degree and hash fields of the key decide."""
    return np.random.default_rng(seed).integers(1, 4, n).astype(np.uint64) << np.uint64(30)


def budget_case(layout):
    """330 partitions on a core of 12 brokers, k <= 1, found by a seed search on the CPU (seeds 0..39 of scaled_instance): the
    winner among 64 orders is order j >= 8 with strictly fewer waves than every earlier order.  (case, j)."""
    if layout == 4:      # count-only: 85 waves at order 42, 86 or more before it
        cur, tgt = scaled_instance(4, 330, 12, 3)
        return ("budget-4", cur, tgt, None, 0, 1, 5), 42
    if layout == 8:      # sized, k = 0: 32 waves at order 40, 33 or more before it
        cur, tgt = scaled_instance(13, 330, 12, 3)
        return ("budget-8", cur, tgt, tied_sizes(330, 513), 8 * GIB, 0, 14), 40
    cur, tgt = scaled_instance(4, 330, 12, 3)   # sized, k = 1: 82 waves at order 20, 83 or more before it
    return ("budget-12", cur, tgt, tied_sizes(330, 504), 8 * GIB, 1, 5), 20


def brokers_for(case, n_ord):
    """The largest n_brokers <= 65534 at which the planner runs exactly n_ord orders of `case`, or None."""
    sized, k = case[3] is not None, case[5]
    wcap, n_mv = case_cap(case), n_moving(case)
    lo, hi = int(max(case[1][case[1] != NONE].max(), case[2][case[2] != NONE].max())) + 1, 65534
    if wr.order_count(lo, wcap, n_mv, sized, k) < n_ord or wr.order_count(hi, wcap, n_mv, sized, k) > n_ord:
        return None
    while lo < hi:      # order_count does not rise with B: the last B with order_count >= n_ord
        mid = (lo + hi + 1) // 2
        if wr.order_count(mid, wcap, n_mv, sized, k) >= n_ord:
            lo = mid
        else:
            hi = mid - 1
    return lo if wr.order_count(lo, wcap, n_mv, sized, k) == n_ord else None


def star(n_mv, size=None, C=0, k=1):
    """Broker 0 is the source of n_mv partitions, each copied to a broker of its own: n_mv rounds, and at k = 1 n_mv waves."""
    cur = np.array([[0, 1 + p] for p in range(n_mv)], dtype=np.uint16)
    tgt = np.array([[0, 1 + n_mv + p] for p in range(n_mv)], dtype=np.uint16)
    return (f"star-{n_mv}", cur, tgt, None if size is None else np.full(n_mv, size, dtype=np.uint64), C, k, 1)


def brokers_of(case):
    return int(max(case[1][case[1] != NONE].max(), case[2][case[2] != NONE].max())) + 1


def one_order_case():
    """230 partitions that each copy from broker 0 to the same 8 brokers, width 8, k = 1: nine participants of degree 230 give
    wave_cap = 9 * 229 + 1 = 2,062, and 65,534 x 2,062 x 4 bytes is above half the budget: one order, 516 MiB.  Every order
    needs 230 waves here, so the winner is order 0 at any order count; a plan with wave_cap > 2,042 on which the orders differ
    has degrees near 230 on tens of brokers, beyond what the sequential model restates in seconds."""
    cur = np.full((230, 8), NONE, dtype=np.uint16)
    cur[:, 0] = 0
    tgt = np.tile(np.arange(1, 9, dtype=np.uint16), (230, 1))
    return ("one-order", cur, tgt, None, 0, 1, 3)


MID_P, MID_B = 1100, 40
TIB = 1 << 40


@functools.lru_cache(maxsize=None)
def mid_rows():
    """About 1,000 moving partitions on 40 brokers: four workgroups of 256, a largest degree near 90 (several batches of 32)."""
    return scaled_instance(21, MID_P, MID_B, 3)


def mid_case(name):
    cur, tgt = mid_rows()
    rng = np.random.default_rng(99)
    kind, _, caps = name.partition("/")
    if kind == "count":
        return (name, cur, tgt, None, 0, 1, 9)
    if kind == "loguniform":
        size, C = sr.gen_sizes(MID_P, 11, zero_share=0.0), TIB
    elif kind == "equal":
        size, C = np.full(MID_P, GIB, dtype=np.uint64), 8 * GIB
    elif kind == "samecode":    # 2^30 and 2^30 + 1 share a traffic code; C holds eight of the first but not eight of the second
        size, C = (GIB + rng.integers(0, 2, MID_P)).astype(np.uint64), 8 * GIB + 3
    elif kind == "oversized":   # one in sixteen is 20 GiB: above C at every participant
        size, C = np.where(rng.random(MID_P) < 1 / 16, 20 * GIB, GIB).astype(np.uint64), 8 * GIB
    else:                       # "zeros": a tenth of the sizes 0
        size, C = sr.gen_sizes(MID_P, 12, zero_share=0.1), TIB
    C, k = {"C0": (C, 0), "C2": (C, 2), "02": (0, 2)}[caps]
    return (name, cur, tgt, size, C, k, 9)


MID_CASES = ("count", "loguniform/C0", "loguniform/C2", "loguniform/02", "equal/C0", "equal/C2", "equal/02", "samecode/C0",
             "samecode/C2", "samecode/02", "oversized/C0", "oversized/C2", "oversized/02", "zeros/C0", "zeros/C2", "zeros/02")


def _with_sizes(name, cur, tgt, seed):
    """The count-only case (k = 2) and two sized ones on the same rows: sizes 0..3 GiB under C = 4 GiB, k = 0 and k = 2."""
    size = np.random.default_rng(seed + 50).integers(0, 4, cur.shape[0]).astype(np.uint64) << np.uint64(30)
    return [(name + "/count", cur, tgt, None, 0, 2, seed), (name + "/C0", cur, tgt, size, 4 * GIB, 0, seed),
            (name + "/C2", cur, tgt, size, 4 * GIB, 2, seed)]


def _padded(rows, width):
    out = np.full((len(rows), width), NONE, dtype=np.uint16)
    for p, r in enumerate(rows):
        out[p, :len(r)] = r
    return out


def shape_rows(kind, seed=1):
    """(cur, tgt) of the row shapes the bit-for-bit cases of the older files lack."""
    rng = np.random.default_rng(seed)
    if kind == "nine":          # width 8, full rows on 20 brokers; two thirds of the targets share no broker with the current row
        cur, tgt = [], []
        for p in range(30):
            c = rng.choice(20, 8, replace=False)
            free = [b for b in range(20) if b not in c]
            t = rng.choice(free, 8, replace=False) if p % 3 else np.where(rng.random(8) < 0.4, rng.permutation(free)[:8], c)
            cur.append(c)
            tgt.append(t)
        return _padded(cur, 8), _padded(tgt, 8)
    if kind == "padded":        # RF 2 in width 8
        cur, tgt = scaled_instance(seed, 40, 9, 2)
        return _padded(cur, 8), _padded(tgt, 8)
    if kind == "nosource":      # current[p][0] is NONE on two thirds of the rows, followers present; 1 to 3 brokers added
        cur, tgt = [], []
        for p in range(40):
            c = rng.choice(10, 3, replace=False)
            free = [b for b in range(10) if b not in c]
            t = c.copy()
            n_new = 1 + p // 3 % 3
            t[:n_new] = rng.choice(free, n_new, replace=False)
            if p % 3:
                c[0] = NONE
            cur.append(c)
            tgt.append(t)
        return _padded(cur, 4), _padded(tgt, 4)
    if kind == "rfchange":      # RF 2 -> 3 (a broker added), RF 3 -> 2 (dropped only: wave 0; or dropped and one replaced)
        cur, tgt = [], []
        for p in range(40):
            c = rng.choice(9, 3, replace=False)
            free = [b for b in range(9) if b not in c]
            if p % 3 == 0:
                cur.append(c[:2])
                tgt.append(np.append(c[:2], rng.choice(free)) if p % 2 else np.array([c[0], rng.choice(free), c[1]]))
            elif p % 3 == 1:
                cur.append(c)
                tgt.append(c[[0, 2]] if p % 2 else c[:2])
            else:
                cur.append(c)
                tgt.append(np.array([rng.choice(free), c[1]]))
        return _padded(cur, 4), _padded(tgt, 4)
    raise ValueError(kind)


def exact_moving(n_mv, seed=1):
    """n_mv moving partitions of RF 3 on 30 brokers among n_mv + 37 (no multiple of 64 for 255, 256, 257), the others unchanged
    or leader-only, in shuffled positions."""
    rng = np.random.default_rng(seed)
    P = n_mv + 37
    cur = np.array([rng.choice(30, 3, replace=False) for _ in range(P)], dtype=np.uint16)
    tgt = cur.copy()
    where = rng.permutation(P)
    for p in where[:n_mv]:
        free = [b for b in range(30) if b not in cur[p]]
        n_new = int(rng.integers(1, 3))
        tgt[p, rng.choice(3, n_new, replace=False)] = rng.choice(free, n_new, replace=False)
    for p in where[n_mv:n_mv + 10]:
        tgt[p] = np.roll(cur[p], 1)
    return cur, tgt


def shape_cases():
    out = []
    for i, kind in enumerate(("nine", "padded", "nosource", "rfchange")):
        cur, tgt = shape_rows(kind)
        out += _with_sizes(kind, cur, tgt, 20 + i)
    for n_mv in (255, 256, 257):
        cur, tgt = exact_moving(n_mv)
        out += _with_sizes(f"moving{n_mv}", cur, tgt, 30)[:2]
    cur, tgt = shape_rows("padded", 2)
    for seed in (0, 1 << 63, (1 << 64) - 1):
        out += [(f"seed{seed}/" + c[0].split("/")[1],) + c[1:] for c in _with_sizes("", cur, tgt, seed)[:2]]
    return out


SHAPE_NAMES = tuple(c[0] for c in shape_cases())
