"""CPU tests of the schedule of a chunked K-search launch (kao_search_chunk_plan: the host function the session itself calls; needs
no device).  A launch group whose block-map entries exceed the workgroups the device holds at once runs every entry's launch as C
pieces inside one grid: ticket -> (entry, chunk, first iteration, iterations).  Forced (KAO_SEARCH_CHUNKS=N) every entry is chunked,
chunk-major; the automatic rule, for launch groups of two resident rounds of entries or more, chunks only a tail -- the last K entries of the block map, K = one resident round -- and leaves
everything in front of it in one piece, so that the hand-off is paid on K / entries of the work.  What the kernel relies on:
every (entry, chunk) exactly once, an entry's chunks in increasing ticket order (a chunk's predecessor holds a lower ticket: the wait
cannot deadlock), contiguous iteration ranges that sum to the launch, no empty chunk; and the automatic rule leaves one-round launches
and short launches in one piece."""
import itertools

import numpy as np
import pytest

ENTRIES = (1, 3, 1536, 8000)
RESIDENT = (1, 1536, 2048)
ITERS = (1, 5, 19, 512)
FORCED = (0, 1, 2, 4, 8)
AUTO = 4          # kChunkAuto: chunks per entry of the automatic rule
TAIL_PCT = 100    # kChunkTailPct: its tail, in percent of the resident workgroups
MIN_ROUNDS = 2    # kChunkMinRounds: ... only from this many resident rounds of entries on
MIN_ITERS = 64    # kChunkMinIters: ... while every chunk keeps this many iterations


def _expected_chunks(entries, resident, iters, forced):
    """-> (chunks per chunked entry, chunked entries: the last of the block map)"""
    tail = entries
    if forced >= 2:
        c = forced
    elif forced == 0 and entries >= MIN_ROUNDS * resident:
        c = AUTO
        while c > 1 and iters // c < MIN_ITERS:
            c //= 2
        tail = min(entries, max(1, resident * TAIL_PCT // 100))
    else:
        c = 1
    c = max(1, min(c, iters))
    return c, (tail if c > 1 else entries)


@pytest.mark.parametrize("entries,resident", list(itertools.product(ENTRIES, RESIDENT)))
def test_chunk_plan(entries, resident):
    import kafka_assignment_optimizer_amd as kao
    for iters, forced in itertools.product(ITERS, FORCED):
        plan = kao.search_chunk_plan(entries, resident, iters, forced)
        key = (entries, resident, iters, forced)
        n_chunks, tail = _expected_chunks(entries, resident, iters, forced)
        whole = entries - tail
        assert plan.shape == (whole + tail * n_chunks, 4), key
        entry, chunk, first, n = (plan[:, i].astype(np.int64) for i in range(4))
        per_entry = np.bincount(entry, minlength=entries)
        # every (entry, chunk) exactly once: the entries in front of the tail in one piece, the tail's in n_chunks
        assert entry.min() == 0 and entry.max() == entries - 1 and len(np.unique(entry * 256 + chunk)) == len(plan), key
        assert (per_entry[:whole] == 1).all() and (per_entry[whole:] == n_chunks).all(), key
        # an entry's chunks in increasing ticket order: sorted by entry (stable in the ticket), the chunk numbers count up from 0
        order = np.argsort(entry, kind="stable")
        starts = np.concatenate(([0], np.cumsum(per_entry)[:-1]))
        assert (chunk[order] == np.arange(len(plan)) - np.repeat(starts, per_entry)).all(), key
        # iteration ranges contiguous, from 0, summing to the launch; no chunk empty (fewer chunks when iters < C); split evenly
        f, m, c_sorted = first[order], n[order], chunk[order]
        assert (f[c_sorted == 0] == 0).all() and (f[1:][c_sorted[1:] > 0] == (f[:-1] + m[:-1])[c_sorted[1:] > 0]).all(), key
        assert (np.add.reduceat(m, starts) == iters).all() and (m >= 1).all(), key
        chunked = per_entry[entry] > 1
        if chunked.any():
            assert m[chunked[order]].max() - m[chunked[order]].min() <= 1, key
        # the tickets dispatched last, what the device empties on, are last chunks: the last K tickets, K the chunked entries
        assert (chunk[-tail:] == n_chunks - 1).all() and (entry[-tail:] == np.arange(whole, entries)).all(), key
        # an entry's chunks are K tickets apart (with K of a resident round or more the chunk before has finished)
        if n_chunks > 1:
            for e in (whole, entries - 1):
                assert (np.diff(np.flatnonzero(entry == e)) == tail).all(), key
        if forced >= 2:
            assert n_chunks == min(forced, iters) and tail == entries, key
        if forced == 1:
            assert n_chunks == 1, key
        if forced == 0:   # the automatic rule: one-round launches and short launches stay in one piece
            if entries < MIN_ROUNDS * resident or iters < 2 * MIN_ITERS:
                assert n_chunks == 1, key
            else:
                assert n_chunks > 1 and m[chunked[order]].min() >= MIN_ITERS and tail == min(entries, resident), key
        if n_chunks == 1:   # one piece: the launch as it always was
            assert (entry == np.arange(entries)).all() and (first == 0).all() and (n == iters).all(), key


def test_chunk_plan_named_splits():
    import kafka_assignment_optimizer_amd as kao
    assert kao.search_chunk_plan(1, 1536, 19, 4)[:, 2:].tolist() == [[0, 5], [5, 5], [10, 5], [15, 4]]
    assert kao.search_chunk_plan(2, 1536, 11, 2)[:, :].tolist() == [[0, 0, 0, 6], [1, 0, 0, 6], [0, 1, 6, 5], [1, 1, 6, 5]]
    assert kao.search_chunk_plan(1, 1536, 5, 8)[:, 3].tolist() == [1, 1, 1, 1, 1]          # the plan shrinks to five chunks
    bench = kao.search_chunk_plan(8000, 1536, 512, 0)                                       # the benchmark's batch: 1,536 of 8,000 entries chunked
    assert len(bench) == 6464 + 1536 * AUTO and bench[:6464, 3].tolist() == [512] * 6464 and bench[6464:, 3].tolist() == [128] * (1536 * AUTO)
    assert len(kao.search_chunk_plan(8000, 1536, 512, 64)) == 8000 * 64 and len(kao.search_chunk_plan(8000, 1536, 512, 200)) == 8000 * 64
