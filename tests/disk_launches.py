"""The kernel launches of one kao_balance_disk* call (stats[3]), replayed from what the call reports.  The host enqueues rounds in
batches and reads the proposal counts once per batch, so the launches say where the batches ended: a round loop that handles the
end of a descent, max_rounds or the FAST to THOROUGH switch differently on a batch boundary gives another count.

The schedule: k_dk_init and k_dk_finish (only with partitions), k_dk_peak0, k_dk_peak1; the exchange call adds k_dkx_index when a
size is above 0.  A round is RANK, PROPOSE, APPLY, and GRANT under a budget or the exchange PROPOSE in the exchange call.  A batch
is nb = min(batch, max_rounds - r) rounds, all enqueued whether they turn out empty or not; batch is 32, or 4 once a call by
utilisation is THOROUGH.  Such a call goes on at the first empty FAST round, r advanced by the rounds that ran.  nb == 0 is a probe:
RANK, PROPOSE and the exchange PROPOSE.  A budgeted call that max_rounds did not stop ends with a probe of RANK and PROPOSE."""
BATCH, THOROUGH_BATCH = 32, 4


def disk_launches(rounds, max_rounds=0, stopped=False, budget=False, capacity=False, exchange=False, thorough=0, partitions=True, sized=True):
    """rounds = stats[0], stopped = stats[5], thorough = stats[10] of a call by utilisation; partitions: P > 0; sized: a size > 0."""
    n = 2 + (2 if partitions else 0) + (1 if exchange and sized else 0)
    if not partitions:
        return n
    per_round = 4 if budget or exchange else 3
    fast = rounds - thorough          # by utilisation: the rounds before the first empty FAST round
    r, is_thorough, done = 0, False, False
    while not done:
        batch = THOROUGH_BATCH if is_thorough else BATCH
        nb = min(batch, max_rounds - r) if max_rounds > 0 else batch
        if nb == 0:
            n += 3 if exchange else 2
            break
        n += nb * per_round
        ran = min(nb, (fast if capacity and not is_thorough else rounds) - r)
        if ran < nb and capacity and not is_thorough:
            is_thorough = True
            r += ran
        else:
            done = ran < nb
            r += nb
    if budget and not stopped:
        n += 2
    return n
