"""Reference for the disk-usage balance under a byte budget (kao_balance_disk_budget), numpy, no GPU: the rounds
of tests/disk_ref.py with the three additions of the definition, all in terms of the INPUT row set in(p):
  cost    a move (p, j, a -> c) costs size[p] * ([c not in in(p)] - [a not in in(p)]): +size, 0, or -size (a fresh copy goes home), so
          the costs of the applied moves sum to bytes_moved; charge = max(cost, 0); rem = max_bytes - spent at the round's start;
  afford  c is a candidate of slot j only if it is admissible and charge <= rem: size <= rem, or a not in in(p), or c in in(p);
  grant   a winner with charge 0 is applied; one with a charge is applied iff the charges of all winners of the round whose source
          ranks lower (applied or not) plus its own are <= rem.  A refused winner changes nothing.
max_bytes = None is no budget.  Loads and sums stay below 2^62, so int64 holds them; the budget and the spend are Python ints."""
import numpy as np

import disk_ref as dr
from wleaders_ref import code

NONE = dr.NONE


def home_of(rows, B):
    """[P, B] bool: b is in the row."""
    rows = np.asarray(rows, dtype=np.int64)
    home = np.zeros((len(rows), B), dtype=bool)
    pp, jj = np.nonzero(rows != NONE)
    home[pp, rows[pp, jj]] = True
    return home


def fresh_bytes(home, rows, w):
    """disk_ref.set_moves(start, rows, w)[1] with home = home_of(start, B), vectorised: a row's brokers are distinct, so the brokers
    of the final set that the input set did not hold are the held slots whose broker is not home."""
    held = rows != NONE
    fresh = (held & ~home[np.arange(len(rows))[:, None], np.where(held, rows, 0)]).sum(axis=1)
    return int((fresh * w).sum())   # below 2^62


def descend(rows, size, B, rack_of, R, cap=0, move_leaders=True, min_gain=0, max_rounds=0, max_bytes=None):
    """The rounds of the definition.  Returns the dict of disk_ref.descend and: refused (winners the grant rule refused, summed over
    the rounds), spent (== bytes_moved), budget_bound (not stopped by max_rounds, and the end state is not move-stable without a
    budget), max_winners (the most winners any round had) and top_rank (the highest source rank of a winner)."""
    rows = np.array(rows, dtype=np.int64)
    start = rows.copy()
    rk = np.asarray(rack_of, dtype=np.int64)
    P, W = rows.shape
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    assert w.shape == (P,) and (w >= 0).all() and rk.shape == (B,)
    budget = 2 ** 64 - 1 if max_bytes is None else int(max_bytes)
    assert 0 <= budget < 2 ** 64
    S = dr.loads(rows, w, B)
    assert int(S.sum()) < 2 ** 62
    S0 = S.copy()
    ssq = [sum(int(x) ** 2 for x in S)]
    peaks = [int(S.max())]
    rounds = moves = proposals = refused = spent = max_winners = 0
    top_rank = -1
    more = False
    first = 0 if move_leaders else 1
    if P and min_gain < 2 ** 62:
        idx = np.arange(P)
        q = np.arange(B)[None, :]
        wcode = np.uint64(0xFFFF) - code(w)
        home = home_of(start, B)
        while True:
            rem = budget - spent
            fits = w <= min(rem, 2 ** 62)                     # (every size is below 2^62)
            order, rank = dr.ranking(S)
            held = rows != NONE
            safe = np.where(held, rows, 0)
            best_rank = np.full(P, B, dtype=np.int64)
            slot = np.zeros(P, dtype=np.int64)
            dest = np.full(P, -1, dtype=np.int64)
            for j in range(first, W):
                a = safe[:, j]
                r = rank[a][:, None]
                afford = home | (~home[idx, a])[:, None] | fits[:, None]
                adm = (dr.admissible(rows, rk, R, cap, j) & afford)[:, order]   # column = rank
                q1 = dr._first_from_top(adm & (q >= r + 1) & (q <= B - 1 - r))
                q2 = dr._first_from_top(adm & (q >= B - r))
                c = np.full(P, -1, dtype=np.int64)
                for qq in (q2, q1):
                    cc = order[np.maximum(qq, 0)]
                    ok = (qq >= 0) & (S[cc] + w + np.int64(min_gain) < S[a])
                    c = np.where(ok, cc, c)
                ok = held[:, j] & (w > 0) & (c >= 0) & (rank[a] < best_rank)
                best_rank = np.where(ok, rank[a], best_rank)
                slot = np.where(ok, j, slot)
                dest = np.where(ok, c, dest)
            prop = dest >= 0
            if not prop.any():
                break
            if max_rounds > 0 and rounds >= max_rounds:
                more = True
                break
            rounds += 1
            proposals += int(prop.sum())
            a = rows[idx, slot]
            d = np.maximum(dest, 0)
            key = (best_rank.astype(np.uint64) << np.uint64(48)) | (wcode << np.uint64(32)) | idx.astype(np.uint64)
            mk = np.full(B, dr.KEY_NONE, dtype=np.uint64)
            np.minimum.at(mk, a[prop], key[prop])
            np.minimum.at(mk, dest[prop], key[prop])
            win = prop & (mk[a] == key) & (mk[d] == key)
            assert win.any()
            touched = np.concatenate([a[win], dest[win]])
            assert len(np.unique(touched)) == len(touched)
            charge = np.where(win & ~home[idx, d] & home[idx, a], w, 0)
            wi = np.nonzero(win)[0]
            wi = wi[np.argsort(best_rank[wi], kind="stable")]
            assert len(np.unique(best_rank[wi])) == len(wi)    # winners and source ranks correspond one to one
            cum = np.cumsum(charge[wi])
            ok = (charge[wi] == 0) | (cum <= min(rem, 2 ** 62))
            assert ok[0]                                       # the lowest key of all is applied
            max_winners = max(max_winners, len(wi))
            top_rank = max(top_rank, int(best_rank[wi].max()))
            refused += int((~ok).sum())
            go = wi[ok]
            spent += sum(int(x) for x in ((~home[go, dest[go]]).astype(np.int64) - (~home[go, a[go]]).astype(np.int64)) * w[go])
            S[a[go]] -= w[go]
            S[dest[go]] += w[go]
            rows[go, slot[go]] = dest[go]
            moves += len(go)
            assert spent == fresh_bytes(home, rows, w) <= budget
            ssq.append(sum(int(x) ** 2 for x in S))
            peaks.append(int(S.max()))
    assert (S == dr.loads(rows, w, B)).all()
    n_moved, bytes_moved = dr.set_moves(start, rows, w)
    assert spent == bytes_moved
    bound = not more and not dr.stable(rows, w, B, rk, R, cap, move_leaders, min_gain)
    return dict(rows=rows, n_moved=n_moved, bytes_moved=bytes_moved, peak_before=int(S0.max()) if B else 0, peak_after=int(S.max()), rounds=rounds,
                moves=moves, proposals=proposals, more=more, rows_changed=int((rows != start).any(axis=1).sum()) if P else 0,
                brokers_changed=int((S != S0).sum()), ssq=ssq, peaks=peaks, refused=refused, spent=spent, budget_bound=bound,
                max_winners=max_winners, top_rank=top_rank)


def stable_budget(rows, start, size, B, rack_of, R, cap=0, move_leaders=True, min_gain=0, rem=0):
    """disk_ref.stable under the budget: no admissible move (p, j, a -> c) with size > 0 and charge <= rem has
    S(c) + size + min_gain < S(a); the charge is taken against the input rows `start`."""
    rows = np.asarray(rows, dtype=np.int64)
    w = np.asarray(size, dtype=np.int64).reshape(-1)
    if not len(rows) or min_gain >= 2 ** 62:
        return True
    S = dr.loads(rows, w, B)
    home = home_of(start, B)
    fits = w <= min(int(rem), 2 ** 62)
    idx = np.arange(len(rows))
    for j in range(0 if move_leaders else 1, rows.shape[1]):
        held = (rows[:, j] != NONE) & (w > 0)
        a = np.where(held, rows[:, j], 0)
        afford = home | (~home[idx, a])[:, None] | fits[:, None]
        gain = S[None, :] + w[:, None] + np.int64(min_gain) < S[a][:, None]
        if (dr.admissible(rows, rack_of, R, cap, j) & afford & gain & held[:, None]).any():
            return False
    return True
