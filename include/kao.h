/* kao.h -- C ABI of libkao.so, the MI355X (gfx950) solver for the Kafka partition-assignment
 * 0-1 model of killerwhile/kafka-assignment-optimizer.
 *
 * What this boundary replaces.  The reference snapshot (/root/reference = README.md + one
 * image) contains no code, hence no FFI declaration to copy.  Its only solver seam is
 * "lp_solve is used behind the scene to solve the generated linear equation"
 * (README.md:135-136): the generated 0-1 model (README.md:144-185) goes in, one 0/1 value per
 * variable plus the objective comes out.  libkao.so replaces exactly that seam; each entry
 * point below cites the README lines it stands in for.  The structured instance (kao_topic)
 * is the compact form of the same model: variable t<T>b<B>p<P>[_l] (README.md:146,
 * README.md:182-184) == "broker B holds a replica of partition P of topic T [as leader]"
 * == assignment[P*rf + k] == B with k == 0 for the `_l` variable.
 *
 * Conventions: plain C, little-endian integers, caller owns every buffer, the library never
 * frees caller memory, no exceptions cross the ABI, return 0 = success / negative = error
 * (kao_strerror).  One process drives one GPU (kao_init(device)); sessions are independent.
 * Every compute entry point runs on the GPU; there is no CPU fallback -- without a usable
 * device the calls fail with KAO_ERR_NO_DEVICE.
 */
#ifndef KAO_H
#define KAO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KAO_VERSION 103 /* 0.1.3: kao_lp_round (KAO-LP's primal side), later kao_plan_waves and kao_plan_waves_sized (no version bump); 0.1.2: kao_lp_bound, kao_session_set_dual_state (KAO-LP, round 5) */
#define KAO_NONE 0xFFFFu /* "no broker": replica on a broker outside the target set / empty slot */
#define KAO_MAX_RF 8     /* replica slots per partition supported by the gfx950 kernels (RF <= 4: one 128-bit word group per
                            partition; 5..8: two) */
#define KAO_MAX_RACKS 255

enum {
    KAO_OK = 0,
    KAO_ERR_INVALID = -1,     /* bad argument */
    KAO_ERR_UNSUPPORTED = -2, /* RF > KAO_MAX_RF, racks > KAO_MAX_RACKS, broker tables too large for LDS */
    KAO_ERR_NO_DEVICE = -3,   /* no gfx950 device / HIP runtime failure at init */
    KAO_ERR_HIP = -4,         /* HIP runtime error (message via kao_last_error) */
    KAO_ERR_NOMEM = -5,
    KAO_ERR_NOT_INIT = -6
};

enum { /* kao_result.status */
    KAO_STATUS_OPTIMAL_PROVEN = 0,    /* feasible and objective == upper_bound */
    KAO_STATUS_FEASIBLE_BOUND_GAP = 1,/* feasible, objective < upper_bound (bound not tight or not optimal) */
    KAO_STATUS_NO_FEASIBLE = 2,       /* search found no feasible assignment (lp_solve would say "infeasible"
                                         only if truly so; this is not a proof) */
    KAO_STATUS_TIME_LIMIT = 3,        /* feasible, stopped by the time limit before target_objective */
    KAO_STATUS_INFEASIBLE_PROVEN = 4  /* a counting argument (kao_check_infeasible) shows that no assignment satisfies
                                         the rows: what lp_solve reports as "This problem is infeasible" */
};

/* One topic's sub-problem.  Topics are independent in the README model: every variable and
 * row carries the topic prefix t1... (README.md:146-184). */
typedef struct kao_topic {
    int32_t n_brokers;        /* B: size of the TARGET broker set (--broker-list, README.md:48) */
    int32_t n_racks;          /* R <= KAO_MAX_RACKS */
    int32_t n_partitions;     /* P */
    int32_t rf;               /* target replication factor (README.md:148-151), <= KAO_MAX_RF */
    int32_t rf_cur;           /* replication factor of `current` (README.md:9: RF may change) */
    const uint8_t *rack_of;   /* [B] dense rack index of each target broker (README.md:27-29) */
    const uint16_t *current;  /* [P*rf_cur] dense broker index, slot 0 = preferred leader
                                 (README.md:52-63); KAO_NONE = broker not in the target set; a broker may not
                                 appear twice in one partition (KAO_ERR_INVALID) */
    int32_t w[2][2];          /* objective weights w[cur_role][new_role], role 0 leader, 1 follower
                                 (README.md:145-146); default {{4,1},{2,2}}; each 0..1023 and
                                 n_partitions * rf * largest weight < 2^24 */
    /* band right-hand sides; -1 = derive floor/ceil of the average (README.md:159-160,
       164-165, 174-175, 179) */
    int32_t rep_lo, rep_hi;     /* C3 replicas per broker   (README.md:158-161) */
    int32_t lead_lo, lead_hi;   /* C4 leaders per broker    (README.md:163-166) */
    int32_t rack_lo, rack_hi;   /* C6 replicas per rack     (README.md:173-176) */
    int32_t prack_lo, prack_hi; /* C7 replicas per partition per rack (README.md:178-180) */
    /* Optional broker weights (NULL = none): extra objective coefficients on EVERY variable of a broker -- broker_w[b] on
       each replica placed on b (t?b<b>p? and t?b<b>p?_l), broker_wl[b] on each leader (t?b<b>p?_l) -- i.e. plain
       coefficients of the README's `max:` row (README.md:145-146).  0..1023 each.  kao_solve_capped uses them to price
       cluster-wide per-broker caps; K-bound and KAO-CX take them into their priced values (round 3); weighted topics are
       not canonicalised. */
    const int32_t *broker_w;    /* [n_brokers] or NULL */
    const int32_t *broker_wl;   /* [n_brokers] or NULL */
} kao_topic;

typedef struct kao_opts {
    uint64_t seed;            /* search is deterministic in (seed, restarts, iters_per_launch) */
    double time_limit_s;      /* kao_solve: wall-clock limit; <= 0 = default 10 s */
    int32_t restarts;         /* parallel restarts (wavefronts) per topic; <= 0 = auto: one round of resident wavefronts
                                 over all topics, fewer for very large topics (depth over breadth): a session takes four per
                                 compute unit on a topic whose assignment lives in HBM (>= 32,768 replica slots; that fills
                                 every SIMD with a wavefront waiting on global loads), kao_solve one per compute unit */
    int32_t iters_per_launch; /* local-search iterations per K-search launch; <= 0 = 512 (sessions) / 128 (kao_solve) */
    int32_t max_launches;     /* kao_solve: stop after this many launches; <= 0 = unlimited */
    int32_t obj_scale;        /* S in cost = lam*violation - S*objective; <= 0 = 4 */
    int32_t lam_min, lam_max; /* penalty sawtooth bounds; <= 0 = 1 / 40 */
    int32_t period_log2;      /* sawtooth period = 2^(period_log2 + (restart & 3)); <= 0 = per topic by size:
                                 floor(log2(2 * n_partitions * rf)) clamped to 8..16 */
    int32_t stop_at_bound;    /* kao_solve: 1 = stop as soon as every topic is OPTIMAL_PROVEN */
    int32_t profile;          /* 1 = bracket every kernel with HIP events (kao_session_stats) */
    int32_t dual_iters;       /* kao_solve: K-bound (Lagrangian dual bound) iterations per launch for topics whose
                                 feasible incumbent is below the bound; 0 = 128 for the first launch, then adapted to
                                 about 10 ms per launch; < 0 = never run K-bound */
    int32_t elite_period;     /* every elite_period-th K-search launch, restarts that trail their topic's best feasible
                                 objective re-seed from that assignment with probability 1/2 ("go with the winners");
                                 0 = kao_solve: about one penalty period of the largest topic, sessions: never; < 0 = never */
    int32_t use_prices;       /* kao_solve: feed K-bound's multipliers (rounded to quarters) back into K-search as Lagrangian
                                 prices of the broker / rack rows (augmented-Lagrangian search); 0 = yes, < 0 = no */
    int32_t use_cycles;       /* kao_solve: KAO-CX (kao_improve_cycles) on incumbents the search has stopped improving;
                                 0 = yes, < 0 = no */
    int32_t islands;          /* kao_solve, experimental: > 1 = search every topic as this many independent copies (own seed,
                                 restarts, elite, K-bound trajectory, KAO-CX) that share one copy's restart budget and answer
                                 with the best; certificates are shared.  0 / 1 = off (measured: no gain) */
    int32_t schedule;         /* kao_solve / kao_solve_multi: 0 = DETERMINISTIC (default): every decision of the solve loop -- which
                                 incumbents K-bound is aimed at and for how many iterations, when its certificates and prices are
                                 merged, when KAO-CX runs and for how many rounds, when elites are exchanged -- is keyed to counts
                                 of launches / iterations / rounds, never to the clock, so the same (instance, options, seed, device
                                 size) gives the same answer whatever the launch timing; the clock (time_limit_s) only decides when
                                 to stop.  1 = wall-clock adaptive (round-2 behaviour: K-bound merged whenever it has finished,
                                 launch lengths adapted to measured times, KAO-CX in time slices): a few percent more work per
                                 second, answers on large topics vary by a unit or two between runs */
    int32_t team;             /* topics whose assignment lives in global memory (beyond ~9,000 partitions): wavefronts that search
                                 ONE restart together (k_team: every wavefront proposes a move per iteration against the same
                                 state, proposals that share no partition / broker / rack with a lower-numbered wavefront's are
                                 all applied).  0 / 1 = one wavefront per restart (k_search; the default: measured on 1000 x 30000 and
                                 1000 x 100000, teams bought neither iterations per second nor a better incumbent in 3 s),
                                 2..8 = team size (4 at most for RF 5..8).  Deterministic either way; other values are KAO_ERR_INVALID.  (Was reserved0.) */
    const int64_t *target_objective; /* kao_solve: optional [n_topics]; a topic counts as done once its feasible
                                        objective reaches this value (e.g. a known optimum); NULL = use the bound */
} kao_opts;

typedef struct kao_result {
    int32_t status;            /* KAO_STATUS_* */
    int32_t best_restart;      /* which restart produced the answer (-1: adopted from another GPU, kao_solve_multi) */
    int64_t objective;         /* value of the README objective (README.md:145-146) */
    int64_t upper_bound;       /* min(closed-form bound (kao_upper_bound), K-bound dual certificate) */
    int32_t violations[8];     /* [0] total, [1..7] = C1..C7 magnitudes of the returned assignment */
    double seconds_to_best;    /* wall time from entry to the launch that produced `objective` */
    uint16_t *assignment;      /* [P*rf] caller-allocated; dense broker index, slot 0 = leader */
} kao_result;

typedef struct kao_stats {
    uint64_t launches;          /* K-search launches */
    uint64_t delta_candidates;  /* neighbours delta-evaluated by K-search, per restart and iteration: REPLACE = all B
                                   brokers of one slot (scan blocks; of TWO slots on topics of at most 24,576 replica slots --
                                   counted as 2 B although the second slot is scanned only when a second lane takes part in
                                   the tournament: an upper bound on small tournaments) or 64 lanes x 4 (sample blocks),
                                   EXCHANGE = all P*rf partner slots, LEADER-SWAP = 64 x (rf-1) */
    uint64_t full_candidates;   /* complete candidates fully evaluated by K-eval */
    double ms_search;           /* HIP-event time of K-search launches (profile=1) */
    double ms_eval;             /* HIP-event time of K-eval launches (profile=1) */
    uint64_t search_bytes_algo; /* algorithmic bytes of the K-search launches */
    uint64_t eval_bytes_algo;   /* algorithmic bytes of the K-eval launches */
    int32_t n_restarts_total;
    int32_t lds_bytes_search;   /* dynamic LDS per K-search workgroup (largest launch group) */
    int32_t blocks_search;      /* workgroups per K-search launch */
    int32_t drift;              /* restarts whose incrementally tracked (V, objective) disagreed with the
                                   from-scratch recount at the end of a launch; must be 0 */
    int32_t launch_groups;      /* topics are bucketed by LDS footprint; one K-search + K-eval launch per group */
    int32_t search_rf3_launches;/* K-search launches (one per launch group and step) that ran the RF-3 instantiation: every topic of
                                   the group has RF 3 and at most 3 current replicas, LDS-resident, unpriced.  Was `reserved`. */
} kao_stats;

typedef struct kao_session kao_session;
typedef struct kao_eval_plan kao_eval_plan;

/* ---- lifetime ------------------------------------------------------------------------- */
int kao_init(int device);            /* select the HIP device of this process; idempotent */
void kao_shutdown(void);
int kao_version(void);
const char *kao_strerror(int code);  /* static storage */
const char *kao_last_error(void);    /* thread-local detail of the last failure */
int kao_device_name(char *buf, int len);

/* ---- host-side model helpers (no device work) ------------------------------------------ */
/* Fill the derived band values (out[0..7] = rep_lo,rep_hi,lead_lo,lead_hi,rack_lo,rack_hi,
 * prack_lo,prack_hi), honouring overrides >= 0.  README.md:158-180. */
int kao_derive_bounds(const kao_topic *t, int32_t out[8]);
/* Upper bound on the objective: every partition keeps its best surviving replicas (coupling rows dropped),
 * minus the cheapest way to perform the evictions / leader changes the bands force (kao_model.cpp). */
int kao_upper_bound(const kao_topic *t, int64_t *ub);
/* Necessary conditions of the model checked by counting (band capacities per broker / rack / partition).  Returns 1
 * and a reason in `why` (may be NULL) if the topic is provably infeasible, 0 if no condition fails (it may still be
 * infeasible for subtler reasons), < 0 on error. */
int kao_check_infeasible(const kao_topic *t, char *why, int why_len);
/* Canonical tie-break among equal-objective feasible assignments (lowest broker index for newly
 * placed replicas, retained followers keep their order): reproduces README.md:88 `[8,1]`.
 * Runs on the GPU (k_canon: the REPLACE scan with "violation delta == 0" as the filter); any topic size. */
int kao_canonicalize(const kao_topic *t, uint16_t *assignment);

/* ---- K-eval: full evaluation of complete candidates (README.md:145-180 in one pass) ---- */
/* One candidate from host memory.  Stands in for "substitute the 0/1 vector into every row of
 * the generated model".  Per-broker counters are 16 + 16 bits (replicas | leaders): a candidate that puts more than
 * 65,535 replicas on one broker (possible only when P*RF > 65535) is reported as KAO_ERR_UNSUPPORTED, never mis-counted. */
int kao_evaluate(const kao_topic *t, const uint16_t *assignment, int64_t *objective, int32_t violations[8]);
/* n candidates [n][P*rf] from host memory; objective[n], violations[n*8]. */
int kao_evaluate_batch(const kao_topic *t, const uint16_t *candidates, int64_t n, int32_t *objective,
                       int32_t *violations);
/* Device-resident batches: tables uploaded once, candidates/outputs are DEVICE pointers. */
int kao_eval_plan_create(const kao_topic *t, kao_eval_plan **out);
int kao_eval_plan_run(kao_eval_plan *p, const void *d_candidates, int64_t n, void *d_objective /* int32[n] */,
                      void *d_violations /* int32[n*8] or NULL */, void *d_best_key /* uint64[1] or NULL */);
int kao_eval_plan_sync(kao_eval_plan *p, double *ms_last /* HIP-event ms of the last run, or NULL */);
void kao_eval_plan_destroy(kao_eval_plan *p);

/* ---- K-search sessions: resident parallel-restart local search ------------------------- */
/* Replaces lp_solve's solve() (README.md:135-136) for a batch of topics. */
int kao_session_create(const kao_topic *topics, int32_t n_topics, const kao_opts *opts, kao_session **out);
/* One step = one K-search launch (iters_per_launch iterations for every restart of every topic)
 * + one K-eval launch over every restart's best snapshot with the wavefront/block min-reduce
 * into one packed key per topic.  Asynchronous on the session's stream. */
int kao_session_step(kao_session *s);
int kao_session_sync(kao_session *s);
/* Starts a new GENERATION of the population: the next kao_session_step re-initialises every restart of every topic from the
 * current assignment (best insertion; the tie-break hash carries the generation number, so the new population differs from
 * the first), and the best snapshots and packed best keys of the old generation are dropped -- read kao_session_best first.
 * K-bound's state, the search prices and the launch counter carry on.  kao_solve does this when a population has converged
 * on an incumbent it cannot prove optimal (the incumbent itself is kept on the host); also a test hook of the bit-exact
 * replay (oracle/kao_port.c re-initialises the same way). */
int kao_session_new_generation(kao_session *s);
/* Copy back per-topic bests (results[n_topics], assignment buffers caller-allocated). */
int kao_session_best(kao_session *s, kao_result *results);
/* Per-topic packed best keys as the device holds them (uint64[n_topics]); the value a
 * min-allreduce across GPUs operates on: viol(20b) << 44 | (0xFFFFFF - objective) << 20 | restart. */
int kao_session_best_keys(kao_session *s, uint64_t *keys);
/* The same keys where they live: DEVICE pointer to uint64[n_topics] (valid for the session's lifetime; written by K-eval on
 * the session's stream -- kao_session_sync first).  What a one-process-per-GPU host hands to ncclAllReduce(..., ncclMin)
 * without a host round trip (kafka_assignment_optimizer_amd/multigpu.py::allreduce_best_resident). */
int kao_session_device_keys(kao_session *s, void **d_keys);
int kao_session_stats(kao_session *s, kao_stats *out);
/* K-search launches so far (of those counted in kao_stats.search_rf3_launches) that ran the small-cost form of the RF-3
 * instantiation: the host has shown from lam_max, obj_scale and the topics' role weights that no move cost of the launch leaves 16 bits
 * (8 lam_max + 4 obj_scale max|w| <= 16384, unpriced), so the kernel forms costs without the clamp and two at a time.  Same results
 * either way; the environment variable KAO_SEARCH_SMALL=0 (read when the session is created) keeps the count at 0. */
int kao_session_small_launches(kao_session *s, int64_t *out);
/* K-search launches so far that ran as ticketed chunks: a launch group with at least twice as many
 * block-map entries as the device holds workgroups at once runs entries' launches as C shorter pieces inside one grid, handed on through global memory, so
 * that the work dispatched last -- what the device empties on -- comes in pieces of 1 / C.  Only the LDS-resident, non-team K-search
 * kernels chunk; topics in global memory, teams and K-init never do.  Same results either way, bit for bit.  The environment variable
 * KAO_SEARCH_CHUNKS (read when the session is created): unset or 0 = the automatic rule (kao_search_chunk_plan; applied only to launch
 * groups that run the small-cost RF-3 kernel on topics below 512 replica slots, the kernel it was measured on), 1 = never,
 * N >= 2 (at most 64) = N uniform chunks on every eligible launch whatever its size.  The schedule is planned once, when the session
 * is created: a step with another iteration count, and every step after prices were switched on in a session created without them
 * (kao_session_set_prices, K-bound's export), launches in one piece -- this counter says what ran.  A chunk that gave up waiting for the one before
 * it (never seen; the wait is bounded so that the kernel always ends) makes the next kao_session_sync / kao_session_best_keys /
 * kao_session_best / kao_session_stats fail with KAO_ERR_HIP -- and every one after it: the error is never cleared, the session's
 * restart states are no longer those of a whole launch and the session can only be destroyed. */
int kao_session_chunked_launches(kao_session *s, int64_t *out);
/* The schedule of a chunked K-search launch, by the host function the session itself calls (no device needed): `entries` block-map
 * entries, `resident` workgroups the device holds at once, `iters` iterations per launch, `forced` as KAO_SEARCH_CHUNKS.  Returns the
 * number of tickets (= entries when the launch stays in one piece; negative: an error) and, when out != NULL and cap >= that number,
 * out[4 t ..] = (entry, chunk, first iteration, iterations) of ticket t.  The automatic rule chunks only when entries >= 2 x resident
 * (a tail of one resident round behind at least as many entries in one piece) and every chunk keeps at least 64 iterations. */
int kao_search_chunk_plan(int32_t entries, int32_t resident, int32_t iters, int32_t forced, int32_t *out, int32_t cap);
/* K-bound: the optimality certificate beyond the closed-form bound (kao_upper_bound).  lp_solve proves optimality
 * by branch-and-bound over the LP relaxation (README.md:135-136); K-bound instead minimises the Lagrangian dual of
 * the same 0-1 model (README.md:144-185) on the device: rows C3, C4, C6 priced with integer multipliers, rows
 * C1, C2, C5, C7 kept in an exactly solved per-partition subproblem.  Every dual value is an upper bound on the
 * optimum, so floor(min dual) is a certificate whatever the multipliers.
 * One launch runs up to `iters` iterations for every topic i with target[i] >= 0 (the incumbent objective the
 * step length aims at; pass -1 to skip a topic).  Topics outside K-bound's limits (broker and rack tables
 * beyond 160 KiB of LDS: about 8,000 brokers; n_partitions*rf > 2^21 (round 6; 2^20 in rounds 4-5, 2^17 before), or n_partitions*rf*(largest weight) > 2^25; a weight outside 0..255) are skipped.  Asynchronous, on a stream of its own: K-bound
 * occupies one compute unit per topic -- one per 512 partitions when a launch holds a topic of more than 2,048 partitions
 * (then every iteration is a kernel launch of its own, see kao_bound.hip) -- and runs beside K-search (kao_session_step); a
 * new launch first waits for the
 * previous K-bound launch (it continues from the multipliers that one left in HBM). */
int kao_session_bound_step(kao_session *s, const int64_t *target, int32_t iters);
/* Search prices.  K-search can carry Lagrangian prices of the coupling rows in its move cost: delta = lam * dViolation
 * - S * dObjective + S * dPrice.  A row's multiplier (a[b]: replicas on broker b, l[b]: leaders on b, g[r]: replicas in rack
 * r) is charged for a unit that enters the row and refunded for one that leaves, but only where the row's count leaves or
 * re-enters its band -- exactly where the violation changes (inside a slack band a unit is free): broker-, rack- and
 * direction-specific penalty weights lam +- multiplier.  With near-optimal multipliers the chain steps an improvement
 * needs (objective down a little, excess moved to another broker) become neutral moves.
 * kao_session_set_prices: a[n_brokers], l[n_brokers], g[n_racks] of one topic from the host (fixed point, 65536 = 1; any
 * values are valid -- prices steer the search, they never change what is reported).  kao_session_adopt_prices: use what
 * the last finished K-bound launch exported (the multipliers of its record dual value, rounded to the quarter grid) for every topic it covered;
 * waits for the K-bound launch in flight.  Both take effect from the next kao_session_step. */
int kao_session_set_prices(kao_session *s, int32_t topic, const int32_t *a, const int32_t *l, const int32_t *g);
int kao_session_adopt_prices(kao_session *s);
/* Test hook: the prices K-search currently carries for one topic (zeros until set or adopted); outputs may be NULL. */
int kao_session_prices(kao_session *s, int32_t topic, int32_t *a, int32_t *l, int32_t *g);
/* 1 while a K-bound launch is still running, 0 when none is (its results can be read without waiting), < 0 = error. */
int kao_session_bound_busy(kao_session *s);
/* Wait for the K-bound launch in flight (if any) and read the certificates back: upper_bound[i] = min(closed-form bound, floor(best dual value));
 * flags[i]: 1 = the last K-bound launch closed the gap to its target, 2 = dual optimum reached (zero subgradient),
 * 4 = no bound (a partition subproblem is infeasible), 8 = topic outside K-bound's limits; iters[i] = K-bound
 * iterations so far.  Any output pointer may be NULL. */
int kao_session_bounds(kao_session *s, int64_t *upper_bound, int32_t *flags, int32_t *iters);
/* Test hook: K-bound state of one topic -- multipliers a[n_brokers], l[n_brokers], g[n_racks] (fixed point, 65536 = 1)
 * and the smallest dual value so far in the same fixed point (INT64_MAX-like before the first iteration). */
int kao_session_dual_state(kao_session *s, int32_t topic, int32_t *a, int32_t *l, int32_t *g, int64_t *best_dual);
/* Test hook / KAO-LP: overwrite K-bound's current multipliers of one topic (a[n_brokers], l[n_brokers], g[n_racks], fixed point
 * 65536 = 1, each clamped to +-2^26); the direction memory and the level control start afresh, the record dual value and the
 * certificate stay.  The next kao_session_bound_step evaluates the dual function there (after the common shifts) and goes on
 * from there.  Waits for a K-bound launch in flight. */
int kao_session_set_dual_state(kao_session *s, int32_t topic, const int32_t *a, const int32_t *l, const int32_t *g);
/* KAO-LP: the certificate from the model's LP relaxation (round 5).  lp_solve's proof of optimality rests on the LP relaxation of
 * the generated model (README.md:135-136, README.md:144-185); K-bound's subgradient iteration approaches that LP's value from
 * above and stalls short of it on slack-band and on large topics.  kao_lp_bound solves the LP itself on the device -- in compact
 * form (new placements pooled per partition and rack; oracle/kao_lp.py states the rows) by a block-structured interior-point
 * method (kao_lp.hip) -- takes its row duals as multipliers, rounds them to K-bound's fixed point and lets K-bound evaluate the
 * dual function there IN INTEGERS: *bound = floor(that value) is a valid upper bound on the optimum whatever the floating-point
 * solve did.  multipliers (may be NULL): a[n_brokers], l[n_brokers], g[n_racks]; stats (may be NULL): [0] interior-point
 * iterations, [1] README objective of the primal iterate, [2] of the dual iterate (the LP value to ~1e-7), [3] 0 converged /
 * 1 iteration limit / 3 stalled (the last finite iterate was used), [4] mu, [5] / [6] relative primal / dual infeasibility,
 * [7] milliseconds of the interior-point solve.  tol <= 0: 1e-7; max_iters <= 0: 80.  KAO_ERR_UNSUPPORTED: outside K-bound's
 * limits or more than ~4,700 brokers. */
int kao_lp_bound(const kao_topic *t, double tol, int32_t max_iters, int64_t *bound, int64_t *best_dual, int32_t *multipliers, double stats[8]);
/* Test hook: the interior-point solve alone, with its trace -- trace[5 * i .. 5 * i + 4] = (mu, primal objective, dual objective,
 * relative primal infeasibility, relative dual infeasibility) of iterate i in the LP's min form (README objective = -value),
 * room for max_iters + 2 iterates; stats and multipliers as kao_lp_bound (any may be NULL).  The parity tests hold the trace against
 * oracle/kao_lp_port.c's. */
int kao_lp_trace(const kao_topic *t, double tol, int32_t max_iters, double *trace, double stats[8], int32_t *multipliers);
/* KAO-LP, the primal side (round 5): an assignment from the LP relaxation.  lp_solve returns the optimum of the generated model
 * (README.md:135-136); on every topic measured the model's LP (README.md:144-185, all rows relaxed to [0, 1]) has INTEGRAL optimal
 * vertices that attain it -- but its optimal face is huge (ties everywhere) and an interior-point iterate ends at the face's
 * analytic centre, fractional in most partitions.  kao_lp_round perturbs the costs by pert * h(variable, salt), h in [0, 1) a
 * hash, which leaves (generically) one optimal vertex; the iterate converges to it, is rounded on the host (new replicas of a rack
 * handed to that rack's brokers by their inflows; specification oracle/kao_lp.py round_primal) and evaluated exactly by K-eval.
 * assignment [P*rf] (dense broker indices, leader first) is overwritten: on entry it may hold a FALLBACK -- the rows that partitions
 * with fractional variables keep (use_fallback != 0; e.g. an incumbent) --, otherwise such partitions are completed together (a search
 * over which current replicas they keep, DESIGN.md section 4b''; far from a vertex: their heaviest options).
 * The result can violate band rows when partitions were fractional: violations[8] as kao_evaluate (violations[0] = total).
 * pert <= 0: min(1e-2, 100 / (P * rf)); tol <= 0: 1e-8; max_iters <= 0: 150.  stats (may be NULL): [0] interior-point iterations,
 * [1] status (0 converged / 1 iteration limit / 3 stalled), [2] fractional partitions, [3] replicas placed beyond a broker's
 * inflow, [4] rows taken from the fallback, [5] milliseconds of the interior-point solve, [6] milliseconds of the rounding,
 * [7] the perturbation used.  An optimality proof needs kao_lp_bound's certificate beside it (objective == bound). */
int kao_lp_round(const kao_topic *t, double pert, uint32_t salt, double tol, int32_t max_iters, int32_t use_fallback, uint16_t *assignment,
                 int64_t *objective, int32_t violations[8], double stats[8]);
/* Test hook: the host half of kao_lp_round alone -- from a quantised iterate to an assignment (no device needed).  q[(2 rf_cur + 2 R) * P]:
 * centi-units min(250, rint(100 x)) of f_j (row j), l_j (row rf_cur + j), yf_r (row 2 rf_cur + r), yl_r (row 2 rf_cur + R + r), each row P
 * long; zq[2 B]: rint(zf_b), rint(zl_b).  assignment / use_fallback as kao_lp_round; rep[4] = {fractional partitions, placements beyond
 * an inflow, unplaced, rows taken from the fallback}.  use_fallback == 2: only the band repair at the end of the rounding, on the complete
 * assignment passed in (q, zq unused, may be NULL).  The parity tests hold it against oracle/kao_lp.py round_primal / repair_bands on the
 * scalar restatement's iterate. */
int kao_lp_round_host(const kao_topic *t, const uint8_t *q, const int32_t *zq, int32_t use_fallback, uint16_t *assignment, int32_t rep[4]);
/* Test hook: KAO-LP's dense kernels alone (kao_chol.hip) on the caller's symmetric positive definite matrix A[n][n] (row-major, the lower
 * triangle is read; n a multiple of 64, at most 10,240): factor[n][n] = L in the lower triangle and L^T tile-wise in the upper one, linv[n / 64]
 * [64][64] = the inverses of L's diagonal tiles, x[n] = the solution of A x = rhs (rhs NULL: all ones), ms[2] = HIP-event milliseconds of
 * the factorisation and of the two triangular solves (second of two runs).  Any output may be NULL. */
int kao_dense_spd_test(const double *A, int32_t n, const double *rhs, double *factor, double *linv, double *x, double ms[2]);
/* Test hooks: the lookup forms of K-search's band arithmetic, as the kernels build them (kao_search_dev.h), on the host.
 * kao_search_band_row: the six state bits of a band row whose count is c against [lo, hi] -- by the per-topic table when the band fits
 * one (*fits = 1; force_plain = 0), by the arithmetic form otherwise or when force_plain is set.  kao_search_rack_delta: the violation
 * delta of a partition-rack count c (0..8) against [lo, hi] for one more (dec = 0) or one fewer (dec = 1) replica, out of the bit table. */
int kao_search_band_row(int32_t lo, int32_t hi, int32_t c, int32_t force_plain, int32_t *fits);
int kao_search_rack_delta(int32_t lo, int32_t hi, int32_t c, int32_t dec);
/* Test hook (round 6): the LP of ONE topic solved by n_dev SHARDS -- shard r holds the partitions [P r / n_dev, P (r + 1) / n_dev) with their
 * variables and local rows; the 3R + 2B coupling rows and the global variables are replicated; per interior-point iteration the shards'
 * parts of the Schur complement meet in one all-reduce (f64 sum), the coupling right-hand sides in one per solve, the scalar records of the
 * reductions in one each; the Cholesky and the triangular solves run replicated.  `devices` may repeat a device with KAO_RCCL_LOOPBACK=1
 * (logical shards through the loop-back table); distinct devices go through RCCL.  pert as kao_lp_round (0: its default; < 0: the model's
 * own LP).  *bound = the certificate (K-bound's integer dual value at the common row duals), assignment / objective / violations = the
 * rounded iterate as kao_lp_round (assignment may be NULL), stats[8] = {iterations, status, fractional partitions, collectives issued,
 * README objective of the dual iterate, milliseconds of the solve, milliseconds of certificate + rounding, perturbation}.
 * kao_solve_multi races whole solves on a replicated large topic by default and runs this sharded solve instead with KAO_MULTI_LP=shard;
 * unmeasured on more than one GPU. */
int kao_lp_sharded_test(const kao_topic *t, const int32_t *devices, int32_t n_dev, double pert, uint32_t salt, double tol, int32_t max_iters,
                        int64_t *bound, uint16_t *assignment, int64_t *objective, int32_t violations[8], double stats[8]);
/* One-shot K-bound on one topic: `launches` launches of `iters` iterations towards `target`.
 * *bound = floor(best dual / 65536) (not combined with kao_upper_bound); multipliers, if not NULL, receives
 * a[n_brokers], l[n_brokers], g[n_racks]. */
int kao_dual_bound(const kao_topic *t, int64_t target, int32_t iters, int32_t launches, int64_t *bound,
                   int64_t *best_dual, int32_t *iters_done, int32_t *flags, int32_t *multipliers);
/* Test hook: state of one restart -- final[P*rf], best[P*rf] (dense), info = {best_obj, V, obj, accepted}. */
int kao_session_restart_state(kao_session *s, int32_t topic, int32_t restart, uint16_t *final_state,
                              uint16_t *best_state, int32_t info[4]);
void kao_session_destroy(kao_session *s);

/* Whole job: create, step until target/time limit, read back, destroy.  What runs inside (round 5): K-search + K-eval on every topic;
 * K-bound beside them (the certificate of small topics); KAO-CX on stalled incumbents; and for every topic of at least 2,048 replica
 * slots that is not closed at once ONE interior-point solve of the model's LP with slightly perturbed costs (KAO-LP): its row duals
 * become the certificate (and the search prices), its iterate -- rounded as kao_lp_round does -- the incumbent; status OPTIMAL_PROVEN means
 * objective == certificate.  Topics from 32,768 slots get that solve before any K-search launch when time_limit_s >= 1 (huge ones: 1.5).
 * The schedule is keyed to counts, not to the clock (kao_opts.schedule = 0): same input, same seed, same answer. */
int kao_solve(const kao_topic *topics, int32_t n_topics, const kao_opts *opts, kao_result *results);
/* Whole job on several GPUs of ONE process (one host thread drives all of them; launches of every device are enqueued
 * before any is waited for).  devices[n_dev] = HIP device ordinals.
 *   n_topics >= n_dev: topics are independent sub-problems (README.md:146-184) and are dealt to the devices (longest
 *     processing time first by brokers x partitions); no exchange on the data path.
 *   n_topics <  n_dev: every device searches every topic with its own seed; every elite_period launches the packed best
 *     keys are min-allreduced on the device-resident buffers (ncclAllReduce, ncclUint64, ncclMin over xGMI) and each topic's
 *     winning assignment is broadcast (ncclBroadcast), so that trailing restarts on EVERY device re-seed from the global
 *     best; certificates are shared (any device's bound is valid).  K-bound runs on the first device only.
 * Listing a device twice gives logical shards on one device (the same flow through plain copies; for tests on one GPU).
 * librccl.so is loaded on first use.  Results as kao_solve. */
int kao_solve_multi(const kao_topic *topics, int32_t n_topics, const int32_t *devices, int32_t n_dev, const kao_opts *opts,
                    kao_result *results);
/* Cluster-wide per-broker load caps (BASELINE config 5; SURVEY.md section 8e "when it does NOT shard"): on top of every
 * topic's own rows, sum over ALL topics of the replicas on broker b <= replica_cap[b] (-1 = no cap for b).  All topics must
 * share one broker set (same n_brokers, same dense index).  The caps couple the topics; they are priced: every round solves
 * the topics independently (kao_solve / kao_solve_multi when n_dev > 1) with broker weights M - mu[b], adds up the broker
 * loads of the answers (the step that is an allreduce(SUM, int32[B]) when topics are sharded over processes) and raises mu[b]
 * on overloaded brokers (projected subgradient with a diminishing step; once a round respects every cap its plan is kept as
 * incumbent and the prices are relaxed again to look for a cheaper one).  results[i] = the best plan found that respects
 * the caps (status FEASIBLE_BOUND_GAP / NO_FEASIBLE; objective = README objective without the weights);
 * *lagrangian_bound (may be NULL) = smallest Lagrangian dual value seen (an upper bound on the capped optimum when every
 * topic's priced sub-problem was proven optimal in that round, else INT64_MAX).  devices / n_dev as kao_solve_multi
 * (NULL / 0 = the current device).  When the `max_rounds` price rounds end without a cap-respecting plan, up to max_rounds / 2 further
 * rounds only RAISE prices until a round in which every topic is feasible respects every cap. */
int kao_solve_capped(const kao_topic *topics, int32_t n_topics, const int32_t *replica_cap, const int32_t *devices, int32_t n_dev,
                     const kao_opts *opts, int32_t max_rounds, kao_result *results, int64_t *lagrangian_bound);
/* ---- KAO-CX: cyclic-exchange improvement of a feasible assignment --------------------------------
 * Stands in for nothing in the reference (lp_solve returns the exact optimum, README.md:135-136): it is the intensification
 * step that lets the device reach optima K-search's one- and two-slot moves do not -- on rigid instances (replicas per
 * broker fixed exactly) the last improvements are cyclic exchanges over 4..10 partitions.  From a FEASIBLE `assignment`
 * ([P*rf], overwritten by the improved one): transfer graphs on the brokers (follower moves, role swaps, band slack), cheapest
 * paths of <= 8 edges by three min-plus squarings, improving cycles and seed rows priced by their closures, candidates
 * unrolled into slot changes and scored exactly by K-eval; rounds until nothing improves or `max_rounds` (<= 0: no limit).
 * kao_solve calls it for unproven topics whose search has stalled.  stats (may be NULL): [0] rounds, [1] improving rounds,
 * [2] realisations evaluated, [3] improving ones, [4] candidates priced > 0, [5] compounds merged, [6] objective before,
 * [7] objective after.  Broker weights (kao_topic.broker_w / broker_wl) enter every edge and seed price.
 * KAO_ERR_UNSUPPORTED: rf < 2, rf > 8 or brokers + racks > 2047. */
int kao_improve_cycles(const kao_topic *t, uint16_t *assignment, int32_t max_rounds, int64_t *objective, int32_t stats[8]);
/* Parity hooks of KAO-CX (tests): the cost matrix of `layer` (0 = follower moves, 1 = role swaps) after `level` squarings
 * (0..3) as dist[n*n], n = B + R + 1 (nodes B .. B+R-1 = the racks' slack nodes, B+R = the global slack node; 1 << 17 = none),
 * the midpoints mid[n*n] (level >= 1; may be NULL) and the slot p*rf+k behind every level-0 edge slot[n*n] (0xFFFFFFFF = none;
 * may be NULL). */
int kao_cycle_matrices(const kao_topic *t, const uint16_t *assignment, int32_t layer, int32_t level, int32_t *dist, int32_t *mid,
                       uint32_t *slot);
/* How a squaring of a graph of n = B + R + 1 nodes (1..2048) is launched, by the host function kao_improve_cycles itself calls (no
 * device needed): out = (np, slices, kchunk) -- the row stride (n rounded up to 64), 1 = the unsplit kernel k_cx_square, >= 2 =
 * k_cx_square_part over that many slices of kchunk midpoints (the last may be shorter).  Honours the test hook
 * KAO_CX_SQUARE_SPLIT (unset or 0: the production rule; 1: never split; N >= 2: N slices requested). */
int kao_cycle_square_plan(int32_t n, int32_t out[3]);
/* The seed table table[P * n_cfg * 2] = (total, completing broker) per partition and configuration (oracle/kao_cycle.py
 * gives the numbering); *n_cfg is always set; table may be NULL to query n_cfg only. */
int kao_cycle_seeds(const kao_topic *t, const uint16_t *assignment, int32_t *table, int32_t *n_cfg);
/* Prototype hook of the next KAO-CX layer (host only, no GPU; specification: oracle/kao_cycle_pairs.py): the
 * COMPOUND EDGES of leader-balanced pairs of leader transfers around a feasible `assignment` -- partition p led by u hands the
 * leadership to v, partition q led by v hands it to u (half-moves of objective gain >= gmin each; a generic entering follower
 * may take the broker the partner releases), and a pair whose net replica effect is one unit x -> z is an edge of cost
 * -(gain of both rows).  cost[B*B] (row x, column z; INT32_MAX = none); stats (may be NULL): [0] half-moves, [1] pairs joined,
 * [2] edges, [3] pairs with no net replica effect and a positive gain.  Not used by kao_solve yet. */
int kao_cycle_pair_edges(const kao_topic *t, const uint16_t *assignment, int32_t gmin, int32_t *cost, int64_t stats[4]);

/* ---- Waves: a reassignment plan split for execution ---------------------------------------------
 * Splits the partitions a plan changes into the fewest waves it finds such that no broker takes part in more than
 * `max_per_broker` partition movements in one wave (Cruise Control's "concurrent partition movements per broker").  Rows of
 * `width` (1..KAO_MAX_RF) broker indices per partition, padded with KAO_NONE, over ONE broker index covering the target brokers
 * AND every broker of `current` (a decommissioned broker is still a copy source); partitions of all topics concatenated (the
 * caps are cluster-wide).  Partition p is unchanged when current[p] == target[p] slot for slot: wave[p] = -1.  A changed p
 * that adds no broker (leader order only, replicas removed) moves no data: wave 0, counted against no cap.  Otherwise its
 * participants are the added brokers plus the copy source current[p][0] when that is not KAO_NONE (new followers fetch from
 * the leader; the plan only names the preferred leader), and each wave holds at most max_per_broker partitions of any one
 * participant.  Waves are numbered from 0; *n_waves = 0 when nothing changed.  *lower_bound = max over brokers of
 * ceil(deg(b) / max_per_broker), deg(b) = moving partitions b takes part in (1 when only leader changes, 0 when nothing
 * changed); *n_waves == *lower_bound proves the split optimal.  Balance bands are not enforced on the states between waves.
 * The waves are the best of several first-fit orders run on the GPU; deterministic in (input, seed).  KAO_ERR_INVALID:
 * max_per_broker < 1, width outside 1..KAO_MAX_RF, n_brokers outside 1..65534, a broker index >= n_brokers (other than
 * KAO_NONE), a broker twice in one row, a target row without a broker. */
int kao_plan_waves(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t *current, const uint16_t *target,
                   int32_t max_per_broker, uint64_t seed, int32_t *wave /* [n_partitions] */, int32_t *n_waves, int32_t *lower_bound);

/* Waves capped by the bytes each broker moves.  Classification, participants, wave numbering and the
 * metadata-only rule are those of kao_plan_waves.  size[p] = bytes of partition p (every partition of the plan).  The traffic of
 * moving partition p at participant b, t_p(b), is size[p] at each added broker (it receives one copy) and n_added(p) * size[p]
 * at the source current[p][0] (it sends one copy per added broker).  Byte cap C = max_bytes_per_broker: in every wave the sum of
 * t_p(b) over the wave's partitions is <= C at each broker b, except that a partition with t_p(b) > C at some participant goes
 * into a wave where each of its participants has byte load 0 (the fit test at b is "load == 0 || load + t_p(b) <= C"), so it
 * ends up alone at its brokers apart from partitions that carry 0 bytes there.  Count cap k = max_per_broker as in
 * kao_plan_waves; k = 0: no count cap; C = 0: no byte cap; with both set both hold.  *lower_bound = max over brokers of
 * ceil(deg(b) / k) (k >= 1) and ceil(sum_p min(t_p(b), C) / C) (C >= 1), and 1 when a partition moves, with the metadata-only
 * rule of kao_plan_waves;
 * *n_waves == *lower_bound proves the split optimal.  Deterministic in (input, seed).  KAO_ERR_INVALID: everything
 * kao_plan_waves rejects except max_per_broker = 0, and size == NULL, max_per_broker < 0, both caps 0, or some broker's total
 * traffic sum_p t_p(b) reaching 2^62 bytes (checked before any device is used). */
int kao_plan_waves_sized(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t *current, const uint16_t *target,
                         const uint64_t *size /* [n_partitions] bytes */, uint64_t max_bytes_per_broker, int32_t max_per_broker,
                         uint64_t seed, int32_t *wave /* [n_partitions] */, int32_t *n_waves, int32_t *lower_bound);

/* Waves that never overfill a disk.  Everything of kao_plan_waves_sized (classes, participants, t_p(b),
 * both caps, keys and orders, *lower_bound), plus stored[b] = bytes broker b holds now and capacity[b] = bytes it may hold.  Kafka
 * keeps the departing copy until the new one is in sync, so within a wave a broker holds its old bytes plus every arrival.  One
 * priority order is run as a sequence of waves w = 0, 1, ..: occ = stored; the still unplaced moving partitions are visited in key
 * order, and p joins wave w iff the sized fit test passes at every participant and, at every added broker b,
 * size[p] == 0 || occ[b] + arr[b] + size[p] <= capacity[b] (arr = bytes arriving in wave w so far).  At the end of the wave
 * occ[b] += arr[b] - dep[b], dep = size[p] at every broker of current \ target of the wave's partitions: departures free room for
 * the NEXT wave.  The metadata-only partitions stay in wave 0, count against no cap and leave with it.  The first wave that takes
 * no partition and frees no byte ends the order; the partitions left over are stuck, wave[p] = -2: in the state reached none of
 * them fits even alone.  The result is the order with the fewest stuck partitions, then the fewest waves, then the lowest index;
 * *n_waves counts up to the last wave that holds a partition.  max_per_broker = 0 and max_bytes_per_broker = 0 together are
 * allowed: headroom alone then shapes the waves.  With capacity[b] = 2^63 everywhere wave[], *n_waves and *lower_bound are those
 * of kao_plan_waves_sized.  stats (may be NULL): [0] stuck partitions, [1] stuck bytes (sum of n_added(p) * size[p], at most
 * 2^63 - 1), [2] the winning order (-1: nothing moves), [3] orders run, [4] round launches, [5] the least free bytes seen, capacity - occ - arr over
 * (wave, broker that receives bytes) of the winning order, at most 2^63 - 1 (-1: none), [6] its wave, [7] its broker (the first
 * wave, then the lowest broker on ties).  Candidates are compared after the clamp: free values above 2^63 - 1 tie.
 * KAO_ERR_INVALID, checked before any device is used: everything kao_plan_waves_sized
 * rejects except both caps 0, and stored == NULL, capacity == NULL, some stored[b] >= 2^62, or some stored[b] below the sum of
 * size[p] over the changed partitions p that leave b. */
int kao_plan_waves_headroom(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t *current, const uint16_t *target,
                            const uint64_t *size /* [n_partitions] bytes */, const uint64_t *stored /* [n_brokers] bytes */,
                            const uint64_t *capacity /* [n_brokers] bytes */, uint64_t max_bytes_per_broker, int32_t max_per_broker,
                            uint64_t seed, int32_t *wave /* [n_partitions] */, int32_t *n_waves, int32_t *lower_bound,
                            int64_t stats[8] /* may be NULL */);

/* ---- Leaders: leader-only rebalancing ---------------------------------------------------------------
 * The fewest preferred-leader changes that put every broker inside the leader band [lead_lo, lead_hi] (as kao_derive_bounds gives
 * it, overrides honoured), moving no data: the README model with every variable of a broker that holds no replica of the
 * partition fixed to 0.  `assignment` [P*rf] holds COMPLETE rows (every slot a dense index below n_brokers, no broker twice in a
 * row; anything else is KAO_ERR_INVALID, checked before the device is used).  For each partition a leader slot j(p) is chosen and
 * the row is overwritten by itself with slots 0 and j(p) swapped; the other followers keep their places.  *n_changed = the
 * partitions with j(p) != 0, the minimum over all choices that meet the band: the restricted model is a min-cost flow, solved
 * exactly on the GPU by successive shortest paths (parallel relaxation over the P*rf implicit arcs, integers only).
 * *status = KAO_STATUS_OPTIMAL_PROVEN, or KAO_STATUS_INFEASIBLE_PROVEN when no choice of leaders among the replicas meets the band
 * (the assignment is then left untouched and *n_changed = 0); the return code is KAO_OK in both cases.  The result depends on the
 * input alone.  *objective (may be NULL) = the README objective of the returned assignment against t->current, by K-eval.
 * stats (may be NULL): [0] phases, [1] relaxation rounds, [2] augmenting paths, [3] longest path in arcs, [4] sum over brokers of
 * max(0, leaders - lead_hi) before, [5] of max(0, lead_lo - leaders) before, [6] kernel launches, [7] units left unrouted (0 unless
 * infeasible).  Limits: rf <= KAO_MAX_RF, n_brokers <= 65534, P*rf <= 4,000,000 (beyond them: KAO_ERR_UNSUPPORTED, as everywhere). */
int kao_balance_leaders(const kao_topic *t, uint16_t *assignment /* [P*rf] in / out */, int32_t *n_changed,
                        int64_t *objective /* README objective of the result by K-eval; may be NULL */,
                        int32_t *status, int32_t stats[8] /* may be NULL */);

/* ---- Failover: failover-aware follower order -------------------------------------------------------
 * When a broker or a rack goes down Kafka hands each orphaned partition to the first live replica of its list, so the order of
 * the followers decides who inherits the leaders.  Rows of `width` (1..KAO_MAX_RF) entries per partition over ONE broker index,
 * partitions of all topics concatenated (the load a failure shifts is a cluster quantity): row p holds k_p >= 1 distinct dense
 * broker indices < n_brokers followed by width - k_p entries of KAO_NONE (mixed RF by padding); slot 0 is the preferred leader;
 * lead[b] = #{p : rows[p][0] == b}.  Scenarios: n_scen = n_brokers for scope 0, n_racks for scope 1; scenario g takes down
 * D_g = {g} (scope 0) or {b : rack_of[b] == g} (scope 1); every replica is assumed in sync.  Partition p belongs to the one
 * scenario g with rows[p][0] in D_g; its eligible slots are E_p = {j >= 1 : rows[p][j] != KAO_NONE and rows[p][j] not in D_g};
 * with E_p empty p is OFFLINE in g, otherwise it is AFFECTED and e(p) = min E_p is the slot Kafka would elect today.  A choice
 * gives each affected p a slot j(p) in E_p; inherit_g(b) = #{affected p of g : rows[p][j(p)] == b}; peak_g = max over b not in
 * D_g of lead[b] + inherit_g(b) (0 when no broker survives).  peak_before[g] = peak_g at j = e; peak_after[g] = the minimum of
 * peak_g over all choices; reordered[g] = the minimum of #{p : j(p) != e(p)} over the choices that attain peak_after[g]
 * (scenarios of one scope share no partition, so all minima are attained together).  Output rows: for every p with
 * j(p) != e(p) the slots e(p) and j(p) are swapped; nothing else moves, slot 0 never moves, no data moves.  dry_run != 0 leaves
 * the rows untouched and reports everything else as if they had been applied.  scen[5g .. 5g+4] = {affected, offline,
 * peak_before, peak_after, reordered}; *n_reordered = the sum of reordered[g].  stats (may be NULL): [0] scenarios with an
 * affected partition, [1] probes of the peak (full solves, the final min-cost solve included), [2] phases, [3] relaxation rounds,
 * [4] augmenting paths, [5] longest path in arcs, [6] kernel launches, [7] partitions of the largest scenario.
 * Exact: for a fixed cap M scenario g is a min-cost flow (each affected partition sends one unit to a broker of E_p, cost 0 for
 * e(p) and 1 otherwise, broker b takes at most M - lead[b]); M is bisected, every scenario in its own workgroup of one launch.
 * The result depends on the input alone.  Checked on the host before any device is used: KAO_ERR_INVALID for a null pointer
 * (stats excepted), scope outside 0..1, width outside 1..KAO_MAX_RF, n_brokers outside 1..65534, n_racks outside
 * 1..KAO_MAX_RACKS, n_partitions < 0, rack_of[b] >= n_racks, slot 0 not a broker, a broker after a KAO_NONE, an index
 * >= n_brokers, a broker twice in one row; KAO_ERR_UNSUPPORTED for n_partitions * width > 4,000,000 or n_brokers >
 * KAO_FAILOVER_MAX_BROKERS (a scenario's node state, 16 bytes per broker, lives in the LDS of one workgroup). */
#define KAO_FAILOVER_MAX_BROKERS 8000
int kao_failover_order(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of /* [n_brokers] */,
                       int32_t n_partitions, int32_t width, uint16_t *rows /* [n_partitions*width] in / out */,
                       int32_t scope /* 0 = single-broker failures, 1 = rack failures */, int32_t dry_run,
                       int32_t *scen /* [n_scen*5] */, int32_t *n_reordered, int32_t stats[8] /* may be NULL */);

/* ---- Leaders across topics: cluster-wide leader balance ------------------------------------------------
 * kao_balance_leaders balances one topic; a topic's band says nothing about how many partitions of the whole cluster a broker
 * leads.  Rows as for kao_failover_order: `width` (1..KAO_MAX_RF) entries per partition over ONE broker index, the partitions of
 * all topics concatenated, row p = k_p >= 1 distinct dense indices < n_brokers, then KAO_NONE padding; slot 0 is the preferred
 * leader; topic_of[p] in 0..n_topics-1 is the topic of row p.  A choice picks a non-empty slot j(p) per partition;
 * L(b) = #{p : rows[p][j(p)] == b}, L(t,b) the same count within topic t.  It is ADMISSIBLE at cap M when
 * topic_lo[t] <= L(t,b) <= topic_hi[t] for every topic t and every broker b of the index (a broker that holds no replica of t has
 * L(t,b) = 0, so topic_lo[t] > 0 is infeasible there), L(b) >= cluster_lo and L(b) <= M for every broker.
 * *peak_before = max_b L(b) at j = 0.  cluster_hi = -1: *peak_after = the smallest M with an admissible choice (it may exceed
 * *peak_before when the input breaks a band), *n_changed = the minimum of #{p : j(p) != 0} over the choices admissible at that M.
 * cluster_hi >= 0: M = cluster_hi, *n_changed = that minimum at M, *peak_after = max_b L(b) of the chosen rows.  Output rows: the
 * input row with slots 0 and j(p) swapped, the other slots in place; no data moves.  dry_run != 0 leaves the rows untouched and
 * reports the same numbers.  *status = KAO_STATUS_OPTIMAL_PROVEN, or KAO_STATUS_INFEASIBLE_PROVEN when no choice is admissible at
 * any M (at cluster_hi); the rows are then untouched, *n_changed = 0 and *peak_after = *peak_before.  The return code is KAO_OK in
 * both cases.  There is no seed: the result depends on the input alone.
 * Exact: for a fixed M this is a min-cost flow on partition -> (topic, broker) -> broker -> sink (bands on the two inner levels,
 * cost 1 for a slot other than 0), solved on the GPU by successive shortest paths over implicit arcs, integers only; feasibility
 * is monotone in M, so M is bisected over max-flow probes and one min-cost solve runs at the optimum, each from j = 0.
 * stats (may be NULL): [0] probes (full solves, the final min-cost solve included), [1] phases, [2] relaxation rounds,
 * [3] augmenting paths, [4] longest path in arcs, [5] kernel launches, [6] (topic, broker) nodes, [7] units the last failed probe
 * left unrouted (0 otherwise).  Checked on the host before any device is used: KAO_ERR_INVALID for a null pointer (stats
 * excepted), width outside 1..KAO_MAX_RF, n_brokers outside 1..65534, n_partitions < 0, n_topics < 1, topic_of out of range,
 * topic_lo < 0 or topic_lo > topic_hi, cluster_lo < 0, cluster_hi < -1, 0 <= cluster_hi < cluster_lo, slot 0 not a broker, a
 * broker after a KAO_NONE, an index >= n_brokers, a broker twice in one row; KAO_ERR_UNSUPPORTED for n_partitions * width >
 * 4,000,000. */
int kao_balance_leaders_cluster(int32_t n_brokers, int32_t n_partitions, int32_t width,
                                uint16_t *rows /* [n_partitions*width] in / out */,
                                const int32_t *topic_of /* [n_partitions], 0..n_topics-1 */, int32_t n_topics,
                                const int32_t *topic_lo, const int32_t *topic_hi /* [n_topics] */,
                                int32_t cluster_lo, int32_t cluster_hi /* -1 = minimise the peak */, int32_t dry_run,
                                int32_t *n_changed, int32_t *peak_before, int32_t *peak_after, int32_t *status,
                                int32_t stats[8] /* may be NULL */);

/* ---- Leaders weighted by traffic -------------------------------------------------------------------------
 * The entry points above count every partition as one unit; here partition p carries weight[p] (produce / fetch traffic, or its
 * size on disk) and W(b) = the sum of weight[p] over the partitions b leads.  Rows as for kao_failover_order and
 * kao_balance_leaders_cluster: `width` (1..KAO_MAX_RF) entries per partition over ONE broker index, all topics concatenated, row
 * p = k_p >= 1 distinct dense indices < n_brokers, then KAO_NONE padding; slot 0 is the preferred leader.
 * Minimising max_b W(b) is NP-hard, so this is a deterministic descent with a certificate.  Synchronous rounds on a leader slot
 * j(p) per partition (0 at the start), each using the loads as they stand at its start: every partition with weight > 0 and
 * k_p >= 2 takes b* = its other replica with the lowest W (ties: the lowest slot) and, a being its leader, proposes a -> b* iff
 * W(b*) + weight[p] + min_gain < W(a); a proposal wins iff its key (0xFFFF - code(W(a))) << 48 | (0xFFFF - code(weight[p])) << 32 | p
 * (code: a monotone 16-bit logarithmic code) is the lowest of all proposals that touch a and of all that touch b*; all winners are
 * applied together; the rounds end when one has no proposal, or after max_rounds rounds (<= 0: no limit).  Every move lowers the
 * sum of W^2 and leaves both loads below the old W(a): the rounds end and the peak never rises.
 * Output rows: the input row with slots 0 and j(p) swapped, the other slots in place; no data moves.  dry_run != 0 leaves the rows
 * untouched and reports the same numbers.  *n_changed = #{p : j(p) != 0}; *peak_before / *peak_after = max_b W(b) before / after.
 * *lower_bound holds for ANY choice of leaders: with the brokers ranked by final load descending (ties: index ascending), m_p the
 * largest rank in row p, A_k the weight of the rows with m_p < k and forced(b) the weight of the rows whose only replica is b, it
 * is max(max_p weight[p], max_b forced(b), max_k ceil(A_k / k)).  *status = KAO_STATUS_OPTIMAL_PROVEN iff *peak_after ==
 * *lower_bound (the peak is then optimal; the number of changes is not claimed minimal), else KAO_STATUS_FEASIBLE_BOUND_GAP; the
 * return code is KAO_OK either way.  There is no seed: the result depends on the input alone.
 * stats (may be NULL): [0] rounds that had a proposal, [1] moves applied, [2] proposals summed over the rounds, [3] kernel
 * launches, [4] 1 = every round ran in one launch of a single workgroup (small inputs), [5] 1 = stopped by max_rounds with a
 * proposal left, [6] the lowest k that attains the level-set term (0 when that term is below the bound), [7] brokers that lead a
 * partition afterwards.  Checked on the host before any device is used: KAO_ERR_INVALID for a null pointer (stats excepted),
 * width outside 1..KAO_MAX_RF, n_brokers outside 1..65534, n_partitions < 0, slot 0 not a broker, a broker after a KAO_NONE, an
 * index >= n_brokers, a broker twice in one row, weights that sum to 2^62 or more; KAO_ERR_UNSUPPORTED for n_partitions * width >
 * 4,000,000. */
int kao_balance_leaders_weighted(int32_t n_brokers, int32_t n_partitions, int32_t width,
                                 uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *weight /* [n_partitions] */,
                                 uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run,
                                 int32_t *n_changed, uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound,
                                 int32_t *status, int64_t stats[8] /* may be NULL */);
/* Test hook.  kao_balance_leaders_weighted picks its kernel path by size; this sets the calling thread's choice for its later calls:
 * 0 = by size, 1 = the single workgroup (KAO_ERR_UNSUPPORTED from the call when the brokers do not fit its LDS), 2 = one launch
 * pair per round.  Both paths give the same bytes.  Returns the previous choice, or KAO_ERR_INVALID.  It governs
 * kao_balance_leaders_weighted_exchange too. */
int kao_wleaders_test_path(int32_t path);

/* ---- Leaders weighted by traffic, with exchange moves ----------------------------------------------------
 * kao_balance_leaders_weighted stops at a move-stable state: no single leader change closes a gap.  This call goes on from there
 * with EXCHANGES: two partitions that both sit on the brokers a and c, one led by a and one by c, swap their leaders.  A leader
 * change moves no data, so a lower peak costs only a longer election list.  Rows, weights, j(p), W(b), code, min_gain and dry_run
 * are those of kao_balance_leaders_weighted.
 * PI = the partitions by weight descending, then p ascending; fixed for the call.  Each round uses the loads as they stand at its
 * start.  It is a MOVE round of kao_balance_leaders_weighted, unchanged, if any partition has a move proposal, else an EXCHANGE
 * round; the call ends when a round has neither kind of proposal, or after max_rounds rounds of both kinds together (<= 0: no
 * limit).
 * EXCHANGE round: a partition x with weight[x] > 0, two replicas or more and leader a walks its other replicas c by W(c) ascending,
 * ties to the lowest slot.  D = W(a) - W(c); a c with D <= 0 is skipped.  S(a, c) = the sub-list of PI of the partitions y != x with
 * weight[y] > 0 whose row holds both a and c and whose current leader is c.  With delta = weight[x] - weight[y], y PASSES iff
 * delta > 0 and delta + min_gain < D (evaluated without overflow).  The passing y are a contiguous run of S(a, c); it is split at
 * g = the number of its members with 2 weight[y] > 2 weight[x] - D; y_hi = the last passing member before the split, y_lo = the
 * first at or after it; the one with the lower |2 delta - D| is taken, a tie goes to y_lo.  (The split lies inside the passing run:
 * if any y passes, one of the two exists, also for 2 min_gain >= D.)  The first c with a passing y gives the proposal (x, y, a <-> c).
 * Its key is (0xFFFF - code(W(a))) << 48 | (0xFFFF - code(delta)) << 32 | x, and it wins iff that key is the lowest of all exchange
 * proposals that touch a, and likewise at c.  Winners are applied together: W(a) -= delta, W(c) += delta, j(x) = the slot of c in
 * row x, j(y) = the slot of a in row y.  Every role of a partition in a proposal touches its leader's broker and winners share no
 * broker, so no partition is touched twice; the globally lowest key wins, so every round applies something; an exchange lowers
 * the sum of W^2 by 2 delta (D - delta) > 0 and leaves both loads below the old W(a): the rounds end and the peak never rises.
 * The state at the first exchange round is kao_balance_leaders_weighted's end state, so without a max_rounds stop *peak_after is
 * never above that call's, the end state is move-stable and exchange-stable (no pair x led by a, y led by c, both rows holding
 * both brokers, has 0 < delta and delta + min_gain < W(a) - W(c)), and an input whose move-stable state is exchange-stable (all
 * positive weights equal, for one) gets the same bytes from both calls.
 * Outputs, status, return codes and the host checks are those of kao_balance_leaders_weighted.  stats (may be NULL): [0] rounds,
 * [1] changes applied and [2] proposals count both kinds of round; [3]..[7] as there ([5]: stopped by max_rounds with a proposal of
 * either kind left); [8] exchange rounds, [9] exchanges applied, [10] exchange proposals, [11] entries of the pair index (one per
 * partition with weight > 0 and unordered pair of its replicas). */
int kao_balance_leaders_weighted_exchange(int32_t n_brokers, int32_t n_partitions, int32_t width,
                                          uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *weight /* [n_partitions] */,
                                          uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run,
                                          int32_t *n_changed, uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound,
                                          int32_t *status, int64_t stats[12] /* may be NULL */);
/* Measurement hook: the microseconds the calling thread's last kao_balance_leaders_weighted_exchange spent on the host building PI
 * and the pair index (tools/wleaders_time.py reports it as a share of the call). */
int64_t kao_wleaders_last_setup_us(void);

/* ---- Failover weighted by traffic -----------------------------------------------------------------------
 * kao_failover_order counts every orphaned partition as one unit; here partition p carries weight[p] (a uint64_t; the weights sum
 * to less than 2^62).  Rows, scopes, the scenarios D_g, the scenario a partition belongs to, its eligible slots E_p, OFFLINE /
 * AFFECTED and e(p) are exactly those of kao_failover_order.  Wlead(b) = the sum of weight[p] over the partitions with
 * rows[p][0] == b.  For scenario g a choice gives each affected p a slot j(p) in E_p, L_g(b) = Wlead(b) + the sum of weight[p] over
 * the affected p of g with rows[p][j(p)] == b, and peak_g = max of L_g(b) over b not in D_g (0 when no broker survives).
 * Minimising peak_g is restricted-assignment makespan with fixed base loads (NP-hard), so every scenario runs, independently, the
 * deterministic descent of kao_balance_leaders_weighted on L_g, with a lower bound computed beside it.  Start: j = e.  A round uses
 * the loads as they stand at its start: every affected p with weight[p] > 0 and |E_p| >= 2 takes b* = its eligible broker other than
 * the current one a = rows[p][j(p)] with the lowest L_g (ties: the lowest slot) and proposes a -> b* iff
 * L_g(b*) + weight[p] + min_gain < L_g(a); a proposal wins iff its key (0xFFFF - code(L_g(a))) << 48 |
 * (0xFFFF - code(weight[p])) << 32 | p (p = the row index, code as in section 4k) is the lowest of all proposals of the round that
 * touch a and of all that touch b*; all winners are applied together.  A scenario ends when a round has no proposal, or after
 * max_rounds rounds of that scenario (<= 0: no limit).  Every move lowers the sum of L_g^2 and leaves both loads below the old
 * L_g(a): the rounds end and the peak never rises.
 * Output rows: for every p with j(p) != e(p) the slots e(p) and j(p) are swapped; nothing else moves, slot 0 never moves, no data
 * moves.  dry_run != 0 leaves the rows untouched and reports the same numbers.  There is no seed.
 * The lower bound of scenario g holds for ANY choice of slots: with T_g = the surviving brokers eligible for at least one affected
 * partition, ranked by final L_g descending (ties: index ascending), m_p = the largest rank among p's eligible brokers and
 * A_k = the Wlead of the brokers of rank < k + the weight of the affected p with m_p < k, it is the maximum of: Wlead(b) over the
 * surviving b; weight[p] + the smallest Wlead among p's eligible brokers, over the affected p; Wlead(b) + the weight of the
 * partitions whose only eligible broker is b, over b in T_g; ceil(A_k / k) for k = 1..|T_g|.
 * scen[6g .. 6g+5] = {affected, offline, peak_before, peak_after, lower_bound, reordered}, reordered = #{p : j(p) != e(p)} (not
 * claimed minimal); a scenario without an affected partition reports peak_before = peak_after = lower_bound = the survivors' largest
 * Wlead (0 when no broker survives).  *n_reordered = the sum of reordered.  *status = KAO_STATUS_OPTIMAL_PROVEN iff peak_after ==
 * lower_bound in every scenario, else KAO_STATUS_FEASIBLE_BOUND_GAP; the return code is KAO_OK either way.
 * stats (may be NULL): [0] scenarios with an affected partition, [1] rounds that had a proposal, summed over the scenarios,
 * [2] moves applied, [3] proposals, summed, [4] kernel launches, [5] scenarios stopped by max_rounds with a proposal left,
 * [6] scenarios with peak_after == lower_bound (those without an affected partition included), [7] the most rounds any one scenario
 * ran.  Checked on the host before any device is used: everything kao_failover_order checks, with the same limits (4,000,000 slots,
 * KAO_FAILOVER_MAX_BROKERS: the load and one key word per broker, 16 bytes, live in the LDS of the scenario's workgroup), and
 * KAO_ERR_INVALID for weight == NULL, status == NULL or weights that sum to 2^62 or more. */
int kao_failover_order_weighted(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                                uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *weight /* [n_partitions] */,
                                int32_t scope, uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run,
                                uint64_t *scen /* [n_scen*6] */, int32_t *n_reordered, int32_t *status,
                                int64_t stats[8] /* may be NULL */);

/* ---- Disk-usage balance ---------------------------------------------------------------------------------
 * Every planner above treats a replica as one unit or moves no data; here partition p stores size[p] bytes (a uint64_t) on every
 * broker of its row, S(b) = the sum of size[p] over the rows that contain b, and replicas MOVE to lower max_b S(b).  Rows as for
 * kao_failover_order: `width` (1..KAO_MAX_RF) entries per partition over ONE broker index, all topics concatenated, row p = k_p >= 1
 * distinct dense indices < n_brokers, then KAO_NONE padding; slot 0 is the preferred leader; rack_of[b] < n_racks; the sum of
 * k_p * size[p] stays below 2^62.
 * A move takes the replica in slot j of row p from broker a to broker c; the slot keeps its place in the row.  Slot 0 may move only
 * when move_leaders != 0 (the preferred leadership goes with it).  c is admissible for (p, j) iff c is not in row p and
 * (max_per_rack <= 0, or rack_of[c] == rack_of[a], or row p holds fewer than max_per_rack brokers of rack_of[c]): a partition's count
 * in a rack never rises above max(max_per_rack, its count there in the input).
 * Synchronous rounds, each using the loads as they stand at its start.  The brokers are ranked by S descending (ties: index
 * ascending; rank 0 is the heaviest).  Every partition with size[p] > 0 makes at most one proposal: it takes its movable slots in
 * ascending rank of their broker; for slot j on a of rank r, c1 = the first admissible broker among the ranks n_brokers-1-r,
 * n_brokers-2-r, .., r+1, and the proposal is (p, j, a -> c1) iff S(c1) + size[p] + min_gain < S(a); otherwise c2 = the first
 * admissible broker among the ranks n_brokers-1, n_brokers-2, .., n_brokers-r, under the same test; otherwise the next slot.  A
 * proposal wins iff its key rank(a) << 48 | (0xFFFF - code(size[p])) << 32 | p (code: the 16-bit logarithmic code of section 4k) is
 * the lowest of all proposals of the round that touch a and of all that touch its destination; all winners are applied together.
 * The rounds end when one has no proposal, or after max_rounds rounds (<= 0: no limit).  Every move lowers the sum of S^2 and leaves
 * both loads below the old S(a): the rounds end, the peak never rises, and the end state is move-stable (no single admissible move
 * closes a gap of more than min_gain).
 * Rows are rewritten in place; dry_run != 0 leaves them untouched and reports the same numbers.  *n_moved = the sum over p of
 * |final set of row p - input set of row p| (the copies Kafka must make; a replica that left and came back counts 0), *bytes_moved
 * the same sum weighted by size[p]; *peak_before / *peak_after = max_b S(b) before / after.  *lower_bound holds for every outcome
 * the moves can reach: the maximum of (0) max_p size[p], (1) ceil(sum of k_p * size[p] / n_brokers), (2) with move_leaders == 0, the
 * largest sum of the slot-0 replicas of one broker.  *status = KAO_STATUS_OPTIMAL_PROVEN iff *peak_after == *lower_bound, else
 * KAO_STATUS_FEASIBLE_BOUND_GAP; the return code is KAO_OK either way (the proof covers the peak, not the bytes moved).  There is no
 * seed: the result depends on the input alone.
 * stats (may be NULL): [0] rounds that had a proposal, [1] moves applied, [2] proposals summed over the rounds, [3] kernel
 * launches, [4] partitions whose row changed, [5] 1 = stopped by max_rounds with a proposal left, [6] the term that gives the bound
 * (0, 1, 2 as numbered above; the lowest on ties), [7] brokers whose load changed.  Checked on the host before any device is used:
 * KAO_ERR_INVALID for a null pointer (stats excepted), width outside 1..KAO_MAX_RF, n_brokers outside 1..65534, n_racks outside
 * 1..KAO_MAX_RACKS, n_partitions < 0, rack_of[b] >= n_racks, slot 0 not a broker, a broker after a KAO_NONE, an index >= n_brokers,
 * a broker twice in one row, replica sizes that sum to 2^62 or more; KAO_ERR_UNSUPPORTED for n_partitions * width > 4,000,000 or
 * n_brokers > KAO_DISK_MAX_BROKERS (every round ranks the brokers by comparing all pairs). */
#define KAO_DISK_MAX_BROKERS 8000
int kao_balance_disk(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                     uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *size /* [n_partitions] */,
                     int32_t max_per_rack /* <= 0: no rack rule */, int32_t move_leaders, uint64_t min_gain,
                     int32_t max_rounds /* <= 0: no limit */, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                     uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound, int32_t *status,
                     int64_t stats[8] /* may be NULL */);

/* ---- Disk-usage balance under a byte budget ---------------------------------------------------------------
 * kao_balance_disk with a cap on the bytes the whole plan copies.  Everything of kao_balance_disk holds: rows, admissibility, rank,
 * the two walks, key, win, the bound, status, n_moved / bytes_moved.  Three things are added, all in terms of the INPUT row set in(p).
 * COST: a move (p, j, a -> c) costs size[p] * ([c not in in(p)] - [a not in in(p)]): +size[p], 0, or -size[p] (a refund: a replica
 * that was a fresh copy goes home), so the costs of all applied moves sum to exactly *bytes_moved.  charge = max(cost, 0): size[p] iff
 * a is in in(p) and c is not, else 0.  rem = max_bytes - spent at the round's start, spent = the sum of the costs so far.
 * AFFORDABLE: broker c is a candidate of slot j only if it is admissible as before AND charge(p, j, a -> c) <= rem, that is
 * size[p] <= rem, or a not in in(p), or c in in(p).  Both walks still stop at their first candidate (every later one is heavier), so
 * "no proposal from slot j" means that no admissible, affordable broker passes the gain test.
 * GRANT: winners are found as before.  A winner with charge == 0 is applied.  A winner with charge > 0 is applied iff the charges of
 * all winners of the round whose source has a lower rank (applied or not) plus its own charge are <= rem: winners share no broker,
 * so winners and source ranks correspond one to one, and the charged winners that are applied are the longest prefix, heaviest
 * source first, that fits.  A refused winner changes nothing: no row, no load, not spent, not the move count.
 * The round's lowest key has the lowest source rank of all proposals, so its prefix is its own charge, which is <= rem: every round
 * with a proposal applies a move, the sum of S^2 falls, the peak never rises, and spent <= max_bytes after every round.  The end
 * state is stable UNDER THE BUDGET: no admissible move with charge <= max_bytes - *bytes_moved closes a gap of more than min_gain.
 * max_bytes = UINT64_MAX (no budget) gives byte for byte the rows, numbers and stats[0..2], [4..7] of kao_balance_disk;
 * max_bytes = 0 applies nothing.  Every value of max_bytes is valid.
 * stats (may be NULL): [0..7] as for kao_balance_disk (a round is four kernel launches here), [8] winners refused by the grant rule,
 * summed over the rounds, [9] 1 iff the budget is what stopped the descent: it was not stopped by max_rounds, and the final state is
 * not move-stable for an unlimited budget.  Checks, limits and refusals are those of kao_balance_disk. */
int kao_balance_disk_budget(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                            uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *size /* [n_partitions] */,
                            int32_t max_per_rack /* <= 0: no rack rule */, int32_t move_leaders, uint64_t min_gain,
                            uint64_t max_bytes /* UINT64_MAX: no budget */, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run,
                            int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
                            uint64_t *lower_bound, int32_t *status, int64_t stats[10] /* may be NULL */);

/* ---- Disk-usage balance by utilisation ---------------------------------------------------------------------
 * kao_balance_disk_budget for brokers with unequal disks: cap[b] is the bytes of disk broker b has, 1 <= cap[b], the sum of cap[b]
 * below 2^62, and the peak to lower is that of the UTILISATION u(b) = S(b) / cap(b).  max_bytes is as there (UINT64_MAX: no budget).
 * Rows, sizes, S(b), admissibility, the rack rule, move_leaders, the movable slots, key, win rule, grant rule, cost / charge / refund,
 * dry_run and *n_moved / *bytes_moved are those of kao_balance_disk and kao_balance_disk_budget.  Four things change.
 * UTILISATION is never computed as a quotient: x / cx is above y / cy iff S(x) * cap(y) > S(y) * cap(x) in 128-bit unsigned
 * arithmetic (both factors stay below 2^62).
 * RANK: the brokers are ranked by u descending, ties to the lower index; rank 0 is the fullest.
 * GAIN TEST: a move (p, j, a -> c) passes iff (S(c) + size[p] + min_gain) * cap(a) < S(a) * cap(c); if the 64-bit sum on the left
 * overflows the move does not pass.  min_gain is any uint64_t, in bytes at the destination.  With equal capacities this is the test
 * of kao_balance_disk.
 * TWO KINDS OF ROUND.  A FAST round is the round of kao_balance_disk: the two walks, each stopping at its first admissible (and,
 * under a budget, affordable) broker, then the test.  With unequal capacities "every later one is heavier" no longer implies that
 * every later one fails: a fuller but larger broker can pass where the emptiest small one does not.  So once a FAST round has no
 * proposal every later round is THOROUGH: for slot j on a of rank r the walk goes over the ranks n_brokers-1, n_brokers-2, .., r+1
 * and proposes the first admissible (and affordable) broker THAT PASSES THE TEST.  (A broker that passes is strictly emptier than a
 * and so ranks behind it: the walk misses no move.)  The descent ends when a THOROUGH round has no proposal, or after max_rounds
 * rounds of either kind that had a proposal.
 * A winner leaves both of its brokers strictly below the old u(a), and winners share no broker: the utilisations sorted descending
 * fall lexicographically in every round, so the rounds end and the peak utilisation never rises.  (The sum of S^2 may rise: cap 1 /
 * S 10 -> cap 100 / S 500 with size 10 passes.)  Without a budget and with max_rounds <= 0 the end state is move-stable: no
 * admissible single move passes the test; under a budget it is stable for the affordable moves.
 * peak_before[2] / peak_after[2] = {S(b*), cap(b*)} of the broker with the highest utilisation before / after (ties: the lowest
 * index).  lower_bound[2] = {numerator, denominator} of the largest, compared as fractions (the lowest-numbered on ties), of
 * (0) {max_p size[p], max_b cap[b]}, (1) {sum of k_p * size[p], sum of cap[b]}, (2) with move_leaders == 0, {fixed(b), cap(b)} of the
 * broker whose slot-0 bytes fixed(b) have the highest ratio (ties: the lowest index; {0, 1} with move_leaders != 0).
 * *status = KAO_STATUS_OPTIMAL_PROVEN iff peak_after equals lower_bound as fractions, or the INTEGRALITY test passes: the sum over b
 * of (ceil(S* * cap(b) / cap*) - 1) is below the sum of k_p * size[p], {S*, cap*} = peak_after, so no placement puts every broker
 * strictly below the achieved utilisation (with equal capacities: peak == ceil(total / n_brokers)); else
 * KAO_STATUS_FEASIBLE_BOUND_GAP.
 * With all cap[b] equal, whatever the common value, the call gives byte for byte the rows of kao_balance_disk and, with a finite
 * max_bytes, those of kao_balance_disk_budget, the same *n_moved, *bytes_moved, peak_before[0], peak_after[0], *status and
 * stats[0..2], [4], [5], [7..9], and stats[10] == 0.
 * stats (may be NULL): [0..9] as for kao_balance_disk_budget; [0] counts the rounds of either kind that had a proposal; [6] is 0, 1 or
 * 2 as there, or 3 when only the integrality test proves the peak; [9]'s probe is a THOROUGH round without the budget; [10] the
 * THOROUGH rounds that had a proposal.  Checks, limits and refusals are those of kao_balance_disk, and KAO_ERR_INVALID for
 * cap == NULL, a cap[b] == 0, or capacities that sum to 2^62 or more. */
int kao_balance_disk_capacity(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                              uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *size /* [n_partitions] */,
                              const uint64_t *cap /* [n_brokers] */, int32_t max_per_rack /* <= 0: no rack rule */,
                              int32_t move_leaders, uint64_t min_gain, uint64_t max_bytes /* UINT64_MAX: no budget */,
                              int32_t max_rounds /* <= 0: no limit */, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                              uint64_t peak_before[2], uint64_t peak_after[2], uint64_t lower_bound[2], int32_t *status,
                              int64_t stats[11] /* may be NULL */);

/* ---- Disk-usage balance with exchange moves ------------------------------------------------------------------
 * kao_balance_disk ends at a move-stable state; this call goes on from there with EXCHANGES: two replicas of different partitions
 * trade places across a broker pair.  By bytes only: no byte budget, no capacities.  Rows, sizes, S(b), admissibility, the rack rule,
 * move_leaders, the movable slots, rank, order[], code, min_gain, dry_run, *n_moved / *bytes_moved, the lower bound and *status are
 * those of kao_balance_disk (the bound still holds: an exchange keeps every k_p and, without move_leaders, never touches slot 0).
 * PI is the list of the partitions with size > 0, by size descending and then index ascending; it is fixed for the call.  Rounds are
 * synchronous and use the loads and ranks as they stand at the round's start.
 * MOVE round: the move proposals of kao_balance_disk are computed; if there is at least one, the round is exactly a round of that call.
 * EXCHANGE round: only when there is no move proposal.  A partition x with size > 0 takes its movable slots in ascending rank of their
 * broker.  For slot j on a of rank q it walks c over the ranks n_brokers-1, n_brokers-2, .., q+1, lightest first.  c is skipped unless
 * it is admissible for (x, j).  Let D = S(a) - S(c); c is skipped when D <= 0.  M is the sub-list of PI of the partitions y != x that
 * have a movable slot k with row y[k] == c and for which a is admissible for (y, k): a is not in row y, and the rack rule holds for
 * the replica that leaves rack_of[c].  With delta = size[x] - size[y], y PASSES iff delta > 0 and delta + min_gain < D (evaluated
 * without overflow; min_gain is any uint64_t).  The passing members are a contiguous run of M.  It is split at g = the number of its
 * members with 2 * size[y] > 2 * size[x] - D (signed; every term stays below 2^63): y_hi is the last passing member before the
 * split, y_lo the first passing member at or after it; the one with the lower |2 * delta - D| is taken, a tie goes to y_lo.  The first
 * (slot, c) with a passing y gives x's one proposal (x, j, y, k, a <-> c), key = q << 48 | (0xFFFF - code(delta)) << 32 | x.
 * WIN: a proposal wins iff its key is the lowest of all the round's exchange proposals that touch a, of all that touch c, of all that
 * name partition x in either role, and of all that name partition y in either role.  (A partition has several replicas that can each
 * take a role; without the two partition words one row could be written by two winners, and its rack rule checked by neither.)  The
 * globally lowest key wins at all four words, so every round with a proposal applies something.
 * APPLY: winners share no broker and no partition.  For each: S(a) -= delta, S(c) += delta, row x[j] = c, row y[k] = a.  Each
 * exchange lowers the sum of S^2 by 2 * delta * (D - delta) > 0 and leaves both loads below the old S(a): the rounds end and the peak
 * never rises.
 * STOP: when a round has neither kind of proposal, or after max_rounds rounds of both kinds counted together (<= 0: no limit).
 * Without a max_rounds stop the end state is move-stable AND exchange-stable: no (x, j, a), (y, k, c) with both sides admissible has
 * 0 < delta and delta + min_gain < S(a) - S(c).  The state at the first exchange round is kao_balance_disk's end state, so
 * *peak_after is never above that call's; an input whose move-stable state is exchange-stable (all positive sizes equal, for one)
 * gets that call's bytes.
 * stats (may be NULL): [0..7] as for kao_balance_disk (rounds, applied moves and proposals count both kinds, an exchange counts 1; a
 * round is four kernel launches), [8] exchange rounds that had a proposal, [9] exchanges applied, [10] exchange proposals, [11] the
 * peak at the start of the first exchange round, 0 when there was none: what kao_balance_disk ends at.
 * Checks, limits and refusals are those of kao_balance_disk, before any device is used, the rows untouched on error; and
 * KAO_ERR_UNSUPPORTED when n_brokers * ceil(N / 64) > KAO_DISK_EXCHANGE_MAX_WORDS, N = the partitions with size > 0: the call keeps
 * one bit per broker and position of PI (1 GiB at the limit; 1000 brokers x 100,000 partitions need 12.5 MB). */
#define KAO_DISK_EXCHANGE_MAX_WORDS (1ull << 27)
int kao_balance_disk_exchange(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                              uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *size /* [n_partitions] */,
                              int32_t max_per_rack /* <= 0: no rack rule */, int32_t move_leaders, uint64_t min_gain,
                              int32_t max_rounds /* <= 0: no limit */, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                              uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound, int32_t *status,
                              int64_t stats[12] /* may be NULL */);

/* ---- Disk-usage balance that empties brokers ------------------------------------------------------------------
 * kao_balance_disk with a set of DRAINING brokers, drain[b] != 0, that are to end without a replica; the others are LIVE.  D = the
 * number of draining brokers.  By bytes only: no byte budget, no capacities, no exchanges.  Rows, sizes, S(b), rounds on the loads as
 * they stand at the round's start, the two walks, key, bid, win rule, apply, determinism and dry_run are those of kao_balance_disk.
 * Six things change.
 * RANK: draining brokers rank before every live broker; inside each group the order is S descending, then index ascending.  A
 * draining broker of rank r < D is thus paired with the (r+1)-th lightest live broker by the unchanged walks.
 * ADMISSIBLE: a destination c must also have drain[c] == 0.  Nothing ever moves onto a draining broker.
 * MOVABLE: a slot whose broker is draining is always movable: slot 0 even with move_leaders == 0 (the preferred leadership goes with
 * it; once on a live broker it is fixed again), and the slots of a partition with size[p] == 0 (skipped everywhere else, as ever).
 * GAIN: a proposal from a draining source needs no gain test: it ignores min_gain and takes c1 if there is one, else c2.  Live
 * sources are tested as in kao_balance_disk.
 * KEY, WIN, APPLY: unchanged.  The rank in the key makes drain moves beat live moves wherever they meet, and a draining broker gives
 * up one replica per round.
 * END: when a round has no proposal, or after max_rounds rounds.  A round with a drain move lowers the number of replicas on draining
 * brokers; any other round leaves it and lowers the sum of S^2: the rounds end.  The peak may RISE while the drain runs;
 * *peak_before / *peak_after stay max_b S(b) over all brokers.
 * *n_left / *bytes_left = the replicas (and their bytes) still on draining brokers in the final rows.  With stats[5] == 0 each of them
 * has no admissible live destination: its row holds every live broker, or the rack rule forbids every other one.  They are reported,
 * they are no error, and the rack rule is never relaxed.
 * *lower_bound holds for every reachable state with the draining brokers empty: the maximum of (0) max_p size[p], (1)
 * ceil(sum of k_p * size[p] / (n_brokers - D)), (2) with move_leaders == 0, the largest sum of the slot-0 replicas that start on one
 * LIVE broker.  *status = KAO_STATUS_OPTIMAL_PROVEN iff *n_left == 0 and *peak_after == *lower_bound, else
 * KAO_STATUS_FEASIBLE_BOUND_GAP; the return code is KAO_OK either way.
 * D == 0 gives byte for byte the rows, numbers and stats[0..7] of kao_balance_disk, *n_left == 0 and stats[8] == stats[9] == 0.
 * stats (may be NULL): [0..7] as for kao_balance_disk, [8] drain moves applied, [9] the number (from 1) of the last round that applied
 * a drain move, 0 when there was none.  Checks, limits and refusals are those of kao_balance_disk, before any device is used, the rows
 * untouched on error; and KAO_ERR_INVALID for drain == NULL, n_left == NULL, bytes_left == NULL, or D == n_brokers (no live broker). */
int kao_balance_disk_drain(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                           uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *size /* [n_partitions] */,
                           const uint8_t *drain /* [n_brokers], != 0: this broker is to end empty */,
                           int32_t max_per_rack /* <= 0: no rack rule */, int32_t move_leaders, uint64_t min_gain,
                           int32_t max_rounds /* <= 0: no limit */, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                           uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound, int32_t *n_left, uint64_t *bytes_left,
                           int32_t *status, int64_t stats[10] /* may be NULL */);

/* ---- Disk-usage balance inside a replica-count band -----------------------------------------------------------
 * kao_balance_disk (exchange == 0) or kao_balance_disk_exchange (exchange != 0) that keeps the number of replicas per broker inside
 * [count_lo, count_hi].  By bytes only: no byte budget, no capacities, no draining brokers.  Everything of those two calls holds (rows,
 * sizes, S(b), rank, the two walks, the gain test, key, bid, win rule, dry_run, *n_moved / *bytes_moved, the exchange rounds) except
 * what follows.
 * COUNT: n(b) = the number of rows that contain b; partitions of size 0 count too.  Like the loads, the counts are taken as they
 * stand at the round's start.
 * ADMISSIBLE: a destination c must also have n(c) < count_hi.
 * MOVABLE: a slot on a is movable only if also n(a) > count_lo.
 * This is the rack rule's form: the count of a broker never rises above max(count_hi, its input count) and never falls below
 * min(count_lo, its input count).  A broker that starts above the band can give and cannot receive; one that starts below can receive
 * and cannot give.  Nothing is forced: a move still needs its gain, so a band the total replica count cannot satisfy is no error, and
 * the sum over b of max(0, n(b) - count_hi) + max(0, count_lo - n(b)) never rises.
 * MOVE rounds: key, bid, win and apply are unchanged; a winner also does n(a) -= 1, n(c) += 1.  Winners share no broker, so a count
 * changes by at most one per round and the test on the counts of the round's start is never overshot.
 * EXCHANGE rounds (exchange != 0; taken when a round has no move proposal inside the band) are those of kao_balance_disk_exchange,
 * untouched: an exchange keeps every count, so the band says nothing about it.
 * END: as in the two calls (the sum of S^2 falls in every round, the peak never rises).  Without a max_rounds stop the end state has no
 * admissible move inside the band that passes the gain test; with exchange it is exchange-stable as well.
 * *lower_bound and *status: the three terms of kao_balance_disk, unchanged.  They hold for every state the call can reach, because the
 * band only removes moves; the bound knows nothing of the band, so a tight band may leave a gap that no plan inside it can close.
 * count_range = {min_b n(b), max_b n(b)} of the input, then the same two of the final rows.
 * stats (may be NULL, else 14 words): [0..7] as for kao_balance_disk; [8..11] as for kao_balance_disk_exchange, and 0 when
 * exchange == 0; [12] the brokers with n(b) outside [count_lo, count_hi] in the final rows, [13] the same of the input.
 * IDENTITY: with count_lo <= 0 and count_hi >= n_partitions the call gives byte for byte the rows, numbers and stats[0..7] of
 * kao_balance_disk (the counts are built inside that call's own launches, so stats[3] is equal too), with exchange != 0 those and
 * stats[8..11] of kao_balance_disk_exchange; stats[12] == stats[13] == 0.
 * Checks, limits and refusals are those of kao_balance_disk and, with exchange != 0, KAO_DISK_EXCHANGE_MAX_WORDS; and KAO_ERR_INVALID
 * for count_lo < 0, count_hi < count_lo or count_range == NULL; all before any device is used, the rows untouched on error. */
int kao_balance_disk_banded(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                            uint16_t *rows /* [n_partitions*width] in / out */, const uint64_t *size /* [n_partitions] */,
                            int32_t count_lo, int32_t count_hi, int32_t exchange /* != 0: exchange rounds as well */,
                            int32_t max_per_rack /* <= 0: no rack rule */, int32_t move_leaders, uint64_t min_gain,
                            int32_t max_rounds /* <= 0: no limit */, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                            uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound, int32_t count_range[4],
                            int32_t *status, int64_t stats[14] /* may be NULL */);

/* ---- Log-dir balance inside each broker ---------------------------------------------------------------------
 * Every planner above treats a broker as one disk; a JBOD broker has several log dirs and dies on the fullest of them.  Broker b
 * owns the dirs dir_start[b] .. dir_start[b+1]-1 of ONE global dir index (CSR; n_dirs = dir_start[n_brokers]; a broker may own no
 * dir, and at most KAO_LOGDIRS_MAX_DIRS).  Dir d carries base[d] bytes that never move (base == NULL: all 0).  Replica r sits in dir
 * dir[r] and holds size[r] bytes; its broker is the one that owns dir[r] (nothing says which partition a replica belongs to).
 * L(d) = base[d] + the sum of size[r] over the replicas with dir[r] == d.  A move takes replica r from dir a to another dir c OF THE
 * SAME BROKER (Kafka copies disk to disk, no network traffic); the goal per broker is a low max_d L(d) over its dirs.
 * Per broker, independently, synchronous rounds, each using the loads as they stand at its start.  The broker's n dirs are ranked by
 * L descending (ties: dir index ascending; rank 0 is the heaviest, order[q] = the dir of rank q).  Every replica with size[r] > 0 on
 * a broker with n >= 2 makes at most one proposal; a = its dir, q = rank(a): if q < n-1-q, c1 = order[n-1-q] (the i-th heaviest is
 * paired with the i-th lightest) and the proposal is a -> c1 iff L(c1) + size[r] + min_gain < L(a) (evaluated without overflow;
 * min_gain is any uint64_t); otherwise, if q >= 1, c2 = order[n-1], the lightest dir, under the same test; otherwise no proposal.
 * Every dir of the broker is admissible, and if any dir passes the test the lightest one does: "no proposal" means that no single
 * move of r closes a gap of more than min_gain.  A proposal wins iff its key q << 48 | (0xFFFF - code(size[r])) << 32 | r (code: the
 * 16-bit logarithmic code of section 4k; r = the replica's index in the call's arrays; keys are unique) is the lowest of all
 * proposals of the round that touch a and of all that touch its destination; all winners are applied together (they share no dir).
 * A broker stops when a round has no proposal, or after max_rounds rounds of that broker (<= 0: no limit).  Every move lowers the
 * sum of L^2 and leaves both loads below the old L(a): the rounds end, the peak never rises, the end state is move-stable.
 * dir[] is rewritten in place; dry_run != 0 leaves it untouched and reports the same numbers.  *n_moved = the replicas whose final
 * dir differs from their input dir (one that left and came back counts 0), *bytes_moved the same weighted by size; *peak_before /
 * *peak_after = the maximum over all dirs.  per_broker[6b..6b+5] = {peak_before, peak_after, lower_bound, moved, bytes_moved,
 * rounds} of broker b; a broker without dirs reports zeros and counts as proven; one with dirs and no replica reports its largest
 * base three times.  lower_bound holds for every placement of the broker's replicas over its dirs: the maximum of
 * (0) max_r size[r] + min_d base[d] over the broker's replicas (0 with none), (1) ceil((sum of base + sum of size) / n),
 * (2) max_d base[d].  *status = KAO_STATUS_OPTIMAL_PROVEN iff peak_after == lower_bound on every broker, else
 * KAO_STATUS_FEASIBLE_BOUND_GAP; the return code is KAO_OK either way.  There is no seed: the result depends on the input alone.
 * stats (may be NULL): [0] brokers that applied a move, [1] rounds that had a proposal, summed over the brokers, [2] moves applied,
 * [3] proposals summed, [4] kernel launches, [5] brokers stopped by max_rounds with a proposal left, [6] brokers with peak_after ==
 * lower_bound, [7] the most rounds any one broker ran.  Checked on the host before any device is used (dir[] stays as it was):
 * KAO_ERR_INVALID for a null pointer (base and stats excepted), n_brokers outside 1..65534, dir_start[0] != 0 or dir_start
 * decreasing, n_replicas < 0, dir[r] outside 0..n_dirs-1, sum of base + sum of size >= 2^62; KAO_ERR_UNSUPPORTED for a broker with
 * more than KAO_LOGDIRS_MAX_DIRS dirs or n_replicas > 4,000,000. */
#define KAO_LOGDIRS_MAX_DIRS 64   /* dirs of one broker: a wavefront ranks them */
int kao_balance_logdirs(int32_t n_brokers, const int32_t *dir_start /* [n_brokers+1] */, const uint64_t *base /* [n_dirs] or NULL */,
                        int32_t n_replicas, int32_t *dir /* [n_replicas] in / out */, const uint64_t *size /* [n_replicas] */,
                        uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run,
                        int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
                        uint64_t *per_broker /* [n_brokers*6] */, int32_t *status, int64_t stats[8] /* may be NULL */);

/* ---- Log-dir balance with exchange moves --------------------------------------------------------------------
 * kao_balance_logdirs stops at a MOVE-STABLE state: no single move closes a gap.  On the small sub-problems of a broker that is often
 * not the best state; this call is the same descent with a second kind of round that runs only when a move round would find nothing.
 * By bytes only.  Dirs, base, size, L(d), the CSR layout, the checks and the limits are those of kao_balance_logdirs; so are dry_run,
 * rank, order[], the move proposal, its key and the win rule.  Each broker is handled on its own, in synchronous rounds, and every
 * round uses the loads as they stand at its start.
 * MOVE round.  The move proposals of kao_balance_logdirs are computed; if the broker has at least one, this round is exactly a round
 * of kao_balance_logdirs.
 * EXCHANGE round, only when the broker has no move proposal.  PI = the broker's replicas in the order size descending, then r
 * ascending (sizes never change: PI is fixed for the whole call).  Every replica x with size[x] > 0, on dir a of rank q, walks the
 * dirs c of the ranks n-1, n-2, .., q+1 in that order (lightest first).  For a dir c, D = L(a) - L(c); the dir is skipped when
 * D <= 0.  g = the number of the broker's replicas whose size s has 2 s > 2 size[x] - D (signed 64-bit arithmetic; every term stays
 * below 2^63).  The two candidates: y_lo, the first replica of PI at a position >= g that sits on c, and y_hi, the last replica of PI
 * at a position < g that sits on c.  A candidate y PASSES iff, with delta = size[x] - size[y]: size[y] > 0, delta > 0 and
 * delta + min_gain < D (evaluated without overflow; min_gain is any uint64_t).  Of the passing candidates the one with the lower
 * |2 delta - D| is taken; a tie goes to y_lo.  The first dir c of the walk that has a passing candidate gives x's proposal
 * (x, y, a <-> c); x makes at most one proposal.  Its key is q << 48 | (0xFFFF - code(delta)) << 32 | x: the heaviest source, then the
 * largest delta by the 16-bit code of section 4k, then the lowest index; keys are unique.  A proposal wins iff its key is the lowest
 * of all the round's proposals that touch a and of all that touch c.  All winners are applied together: L(a) -= delta,
 * L(c) += delta, dir[x] = c, dir[y] = a.
 * STOP.  A broker stops when a round has neither kind of proposal, or after max_rounds rounds of that broker, both kinds counted
 * (<= 0: no limit).
 * WINNERS ARE DISJOINT.  Winners share no dir.  The partner y of a winner never wins in the same round: its own key carries the rank
 * of c, which is larger than q, so it loses at c.  Hence no replica is touched twice.
 * THE ROUNDS END AND THE PEAK NEVER RISES.  An exchange leaves both loads strictly below the old L(a) and lowers the sum of L^2 by
 * 2 delta (D - delta) > 0.  The globally lowest key wins, so every round with a proposal applies something.
 * COMPLETENESS.  If any y on c passes for x, then one of y_lo / y_hi does: the passing sizes form the interval
 * (size[x] - D + min_gain, size[x]), and the two candidates bracket its midpoint size[x] - D / 2.  So the end state is move-stable AND
 * EXCHANGE-STABLE: no pair of replicas on two dirs of a broker has 0 < delta and delta + min_gain < D.
 * IDENTITY.  The state at the broker's first exchange round is the end state of kao_balance_logdirs, so peak_after here is <= that
 * call's, on every broker.  On an input whose move-stable state is already exchange-stable (all positive sizes equal, for one) the
 * two calls agree in dir[], n_moved, bytes_moved, the peaks and the shared columns.
 * *n_moved, *bytes_moved, *peak_before, *peak_after, *status and the lower_bound terms are as in kao_balance_logdirs; moved counts the
 * replicas whose final dir differs from their input dir.  per_broker[8b..8b+7] = {peak_before, peak_after, lower_bound, moved,
 * bytes_moved, rounds, exchange_rounds, exchanges}.  stats (may be NULL): [0]..[7] those of kao_balance_logdirs, where rounds, moves
 * and proposals count both kinds; [8] exchange rounds summed, [9] exchanges applied, [10] exchange proposals, [11] brokers whose
 * peak an exchange round lowered.  Host checks and error codes are those of kao_balance_logdirs, run before any device is used, and
 * dir[] stays untouched on error. */
int kao_balance_logdirs_exchange(int32_t n_brokers, const int32_t *dir_start /* [n_brokers+1] */, const uint64_t *base /* [n_dirs] or NULL */,
                                 int32_t n_replicas, int32_t *dir /* [n_replicas] in / out */, const uint64_t *size /* [n_replicas] */,
                                 uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run,
                                 int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
                                 uint64_t *per_broker /* [n_brokers*8] */, int32_t *status, int64_t stats[12] /* may be NULL */);
/* Test hook: where kao_balance_logdirs_exchange keeps PI and the dir masks of a broker in THIS thread's calls: 0 = by the largest
 * bucket and the most dirs of the call (the default), 1 = in LDS (the call returns KAO_ERR_UNSUPPORTED when they do not fit), 2 = in
 * global memory.  Returns the previous choice; both paths give the same bytes. */
int kao_logdirs_test_exchange(int32_t path);

/* ---- Log dirs for arriving and evacuated replicas -----------------------------------------------------------
 * Dirs, base, size and L(d) are those of kao_balance_logdirs.  Replica r belongs to broker broker[r].  It is a RESIDENT when
 * dir[r] >= 0, and that dir must be one of broker[r]'s; it is HOMELESS when dir[r] == -1: a replica that a plan brings to the broker,
 * or one whose dir is being evacuated.  Every broker is handled on its own.
 * PLACE.  F(d) = base[d] + the sizes of the residents of d.  The broker's homeless replicas are taken in the order size descending,
 * then r ascending (r = the index in the call's arrays, so the result depends on the input alone); each goes to the dir with the
 * lowest load at that moment (ties: the lowest dir index), whose load grows by its size.  Zero-size replicas are placed the same
 * way and come last.
 * move_residents == 0: the residents stay and no round runs; min_gain and max_rounds are not used.  None is needed: after PLACE no
 * single move of a placed replica closes any gap.  Let r be the LAST replica put on dir a; it went there when a was the lightest
 * dir, so L(a) - size[r] <= L(c) held for every dir c then and holds at the end (loads only grow, and a's only by r's size).  Every
 * earlier replica x on a has size[x] >= size[r], so L(c) + size[x] >= L(c) + size[r] >= L(a): no move a -> c of a placed replica
 * passes the test L(c) + size + min_gain < L(a), even at min_gain 0.
 * move_residents != 0: the rounds of kao_balance_logdirs run from the placed state over ALL replicas of the broker: same rank,
 * pairing, test, key with r, win rule and stop rule.
 * lower_bound of a broker holds for every outcome.  M = the replicas that may change dir (the homeless ones; all with
 * move_residents), F' = the fixed load (F; base with move_residents): the maximum of (0) max_{r in M} size[r] + min_d F'(d) (0 when
 * M is empty), (1) ceil((sum of F' + sum over M of size) / n), (2) max_d F'(d).  *status = KAO_STATUS_OPTIMAL_PROVEN iff peak_after
 * == lower_bound on every broker.
 * *peak_before = max_d F(d) of the input: the homeless replicas are nowhere yet, so *peak_after may exceed it.  *n_placed /
 * *bytes_placed = the homeless replicas and their sizes; *n_moved / *bytes_moved = the RESIDENTS whose final dir differs from their
 * input dir.  per_broker[8b..8b+7] = {peak_before, peak_after, lower_bound, placed, bytes_placed, moved, bytes_moved, rounds}; a
 * broker without dirs reports zeros and counts as proven.  dry_run != 0 leaves dir[] as it was (homeless replicas still at -1) and
 * reports the same numbers.
 * Two identities.  With no homeless replica and move_residents != 0 the call gives byte for byte the dir[], the peaks, n_moved and
 * bytes_moved of kao_balance_logdirs, whose six per_broker columns appear at {0, 1, 2, 5, 6, 7} of the eight.  With no homeless
 * replica and move_residents == 0 nothing changes and every broker is proven.
 * stats (may be NULL): [0] brokers that placed a replica, [1] brokers that applied a move, [2] rounds summed, [3] moves applied,
 * [4] proposals summed, [5] kernel launches, [6] brokers stopped by max_rounds, [7] brokers proven, [8] the most rounds of one
 * broker, [9] the most homeless replicas of one broker.
 * Checked on the host before any device is used (dir[] stays as it was): KAO_ERR_INVALID for every such case of
 * kao_balance_logdirs (dir[r] may be -1 here), a null broker or output pointer, broker[r] outside 0..n_brokers-1, dir[r] below -1
 * or >= n_dirs, a resident whose dir is not its broker's, a homeless replica on a broker without dirs, base and size summing to
 * 2^62 or more; KAO_ERR_UNSUPPORTED for a broker with more than KAO_LOGDIRS_MAX_DIRS dirs or n_replicas > 4,000,000. */
int kao_place_logdirs(int32_t n_brokers, const int32_t *dir_start /* [n_brokers+1] */, const uint64_t *base /* [n_dirs] or NULL */,
                      int32_t n_replicas, const int32_t *broker /* [n_replicas] */, int32_t *dir /* [n_replicas] in / out, -1 = homeless */,
                      const uint64_t *size /* [n_replicas] */, int32_t move_residents, uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */,
                      int32_t dry_run, int32_t *n_placed, uint64_t *bytes_placed, int32_t *n_moved, uint64_t *bytes_moved,
                      uint64_t *peak_before, uint64_t *peak_after, uint64_t *per_broker /* [n_brokers*8] */, int32_t *status,
                      int64_t stats[10] /* may be NULL */);
/* Test hook: how kao_place_logdirs sorts a broker's homeless replicas in THIS thread's calls: 0 = by the largest homeless count of
 * the call (the default), 1 = in LDS (the call returns KAO_ERR_UNSUPPORTED when a broker has more than 4,096), 2 = in global
 * memory.  Returns the previous choice; both paths give the same bytes. */
int kao_logdirs_test_sort(int32_t path);

/* ---- Log-dir planners by utilisation ------------------------------------------------------------------------
 * kao_balance_logdirs and kao_place_logdirs even out bytes; a broker's volumes are often unequal, and it takes a dir offline when
 * that dir fills.  Here cap[d] >= 1 is the bytes of disk behind dir d (the sum over all dirs below 2^62) and the quantity that the
 * moves lower is the UTILISATION u(d) = L(d) / cap(d).  Dirs, base, size, L(d), F(d), residents, homeless replicas, the CSR layout,
 * the limits, the checks, dry_run and the counters are those of the two calls above; only what follows changes.
 * NO QUOTIENT.  x / cx is above y / cy iff x * cy > y * cx in unsigned 128-bit arithmetic (both factors stay below 2^62); a
 * utilisation is never a double or a division in anything that decides a move.
 * RANK.  A broker's dirs are ranked by u descending (ties: dir index ascending; rank 0 is the fullest, order[q] = the dir of rank q).
 * GAIN TEST.  r: a -> c passes iff (L(c) + size[r] + min_gain) * cap(a) < L(a) * cap(c); if the 64-bit sum on the left overflows the
 * move does not pass (min_gain is any uint64_t).
 * PROPOSAL.  Every replica r with size[r] > 0 on a broker with n >= 2 dirs makes at most one; a = its dir, q = rank(a).  If
 * q < n-1-q and c1 = order[n-1-q] passes the test, the proposal is a -> c1.  Otherwise the ranks n-1, n-2, ..., q+1 are walked in
 * that order and the first dir that passes is proposed.  A dir that passes is strictly emptier than a and so ranks behind it: the walk
 * sees every move there is, and "no proposal" means that no single move of r passes the test.  (With bytes, if any dir passes the
 * lightest does; not so here: a fuller but larger dir can pass where the emptiest small one does not.)
 * KEY, WIN RULE, APPLY, STOP RULE: those of kao_balance_logdirs, q being the utilisation rank.  A winner leaves both of its dirs
 * strictly below the old u(a) and winners share no dir, so the broker's utilisations sorted descending fall lexicographically every
 * round: the rounds end, the peak utilisation never rises, the end state is move-stable.  (The sum of L^2 may rise.)
 * PLACE (kao_place_logdirs_capacity).  The homeless replicas are taken size descending, then r ascending; each goes to the dir with
 * the lowest (L(d) + size[r]) / cap(d) at that moment, compared by products (ties: the lowest dir index).  After PLACE no single move
 * of a placed replica passes the test, even at min_gain 0: let r be the LAST replica put on a, L_then the loads just before.  Then
 * u_final(a) = (L_then(a) + size[r]) / cap(a) <= (L_then(c) + size[r]) / cap(c) for every dir c by the choice of a, and for every
 * earlier replica x on a, size[x] >= size[r] and loads only grow, so (L_then(c) + size[r]) / cap(c) <= (L_final(c) + size[x]) / cap(c):
 * the test (L(c) + size[x]) * cap(a) < L(a) * cap(c) fails.  With move_residents != 0 the rounds above run from the placed state over
 * ALL replicas of the broker.
 * BOUND of a broker, a fraction {num, den} that no outcome undercuts.  M = the replicas that may change dir and F' = the fixed loads
 * as for kao_place_logdirs (the balance call: M = every replica, F' = base).  The bound is the largest, as fractions (ties: the
 * lowest-numbered term), of (0) the lowest over d of {F'(d) + max_{r in M} size[r], cap(d)}, and {0, 1} when M is empty; (1) {sum of
 * F' + sum over M of size, sum of cap(d)}; (2) the highest over d of {F'(d), cap(d)}; inside (0) and (2) ties go to the lowest dir.
 * INTEGRALITY TEST, a second proof: {L*, cap*} = the broker's peak after; room(d) = max(0, ceil(L* * cap(d) / cap*) - 1 - F'(d)), each
 * cut at the sum over M of size; the test passes iff the rooms sum to less than that sum: a dir strictly below the achieved
 * utilisation holds at most ceil(L* * cap(d) / cap*) - 1 bytes, so no outcome puts every dir strictly below it.  A broker is PROVEN
 * iff its peak equals the bound as fractions or the test passes; *status = KAO_STATUS_OPTIMAL_PROVEN iff every broker is.  With
 * equal capacities "proven" coincides with peak_after == lower_bound of the byte calls.
 * peak_before[2] / peak_after[2] = {L, cap} of the fullest dir of the call (ties: the lowest global dir index; {0, 1} without dirs;
 * for the place call peak_before is taken over F).  per_broker, balance: [10b..10b+9] = {L_before, cap_before, L_after, cap_after,
 * lb_num, lb_den, moved, bytes_moved, rounds, proof}; place: [12b..12b+11] = {L_before, cap_before, L_after, cap_after, lb_num,
 * lb_den, placed, bytes_placed, moved, bytes_moved, rounds, proof}; proof: 0 = gap, 1 = bound met, 2 = integrality test only.  A
 * broker without dirs reports {0, 1, 0, 1, 0, 1, 0, ..., 0, proof 1}.  stats are those of the byte calls ("proven" by either proof).
 * IDENTITY.  With all cap[d] equal each call gives the dir[], n_moved, bytes_moved, n_placed, bytes_placed, peak_*[0], status, the L,
 * moved, bytes, placed and rounds columns and every stats entry but the launch count of its byte sibling.
 * Checked on the host before any device is used: everything the byte calls check, and KAO_ERR_INVALID for cap == NULL, a cap[d] == 0,
 * or capacities summing to 2^62 or more. */
int kao_balance_logdirs_capacity(int32_t n_brokers, const int32_t *dir_start /* [n_brokers+1] */, const uint64_t *base /* [n_dirs] or NULL */,
                                 const uint64_t *cap /* [n_dirs] */, int32_t n_replicas, int32_t *dir /* [n_replicas] in / out */,
                                 const uint64_t *size /* [n_replicas] */, uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run,
                                 int32_t *n_moved, uint64_t *bytes_moved, uint64_t peak_before[2], uint64_t peak_after[2],
                                 uint64_t *per_broker /* [n_brokers*10] */, int32_t *status, int64_t stats[8] /* may be NULL */);
int kao_place_logdirs_capacity(int32_t n_brokers, const int32_t *dir_start /* [n_brokers+1] */, const uint64_t *base /* [n_dirs] or NULL */,
                               const uint64_t *cap /* [n_dirs] */, int32_t n_replicas, const int32_t *broker /* [n_replicas] */,
                               int32_t *dir /* [n_replicas] in / out, -1 = homeless */, const uint64_t *size /* [n_replicas] */, int32_t move_residents,
                               uint64_t min_gain, int32_t max_rounds /* <= 0: no limit */, int32_t dry_run, int32_t *n_placed, uint64_t *bytes_placed,
                               int32_t *n_moved, uint64_t *bytes_moved, uint64_t peak_before[2], uint64_t peak_after[2],
                               uint64_t *per_broker /* [n_brokers*12] */, int32_t *status, int64_t stats[10] /* may be NULL */);

/* Diagnostic: runs the two collectives kao_solve_multi uses (ncclAllReduce(ncclUint64, ncclMin) and ncclBroadcast) on
 * small resident buffers of the listed distinct devices and checks the results.  0 = ok. */
int kao_rccl_selftest(const int32_t *devices, int32_t n_dev);
/* Test hook.  With KAO_RCCL_LOOPBACK=1 in the environment kao_solve_multi and kao_rccl_selftest take their collectives from an
 * in-process loop-back table instead of librccl: the device list may then name one device several times ("ranks" on one GPU)
 * and the grouped ncclAllReduce(ncclUint64, ncclMin) / ncclBroadcast call sequence of the elite exchange runs exactly as it
 * does between distinct GPUs, the data moving through plain copies when a group closes.  out[0] / out[1] = all-reduces /
 * broadcasts the loop-back table has completed in this process. */
int kao_rccl_loopback_counts(uint64_t out[2]);
/* Wall-clock breakdown of this thread's last kao_solve / kao_solve_multi, seconds from its entry:
 * out[0] session ready (instance prepared + uploaded), out[1] last improving launch finished (time-to-best),
 * out[2] results read back, out[3] returned (buffers released); out[4] = launches run; out[5] = neighbours K-search
 * delta-evaluated in those launches (kao_stats.delta_candidates, all devices), out[6] = K-bound launches, out[7] = elite
 * exchanges between GPUs (kao_solve_multi), out[8] = K-bound iterations summed over the topics, out[9] = KAO-CX calls,
 * out[10] = KAO-CX calls that improved an incumbent, out[11] = K-search iterations per restart, out[12] = generations started
 * after the first (kao_session_new_generation), out[13] = KAO-CX runs from further starting points (other restarts' best
 * snapshots; included in out[9]), out[14] = KAO-LP solves that delivered multipliers, out[15] = their interior-point iterations. */
int kao_last_solve_timing(double out[16]);
/* KAO-LP in this thread's last kao_solve: out[0] solves that delivered multipliers, out[1] their interior-point iterations, out[2] iterates
 * rounded into an assignment (kao_lp_round's primal side inside the solve), out[3] of those adopted as a topic's incumbent, out[4]
 * partitions with fractional variables summed over the rounded iterates; out[5..7] reserved (0). */
int kao_last_solve_lp(double out[8]);
/* K-search as THIS thread's last kao_solve ran it (only when that solve had kao_opts.profile = 1: every K-search / K-eval launch is
 * then bracketed by HIP events on the session's stream): out[0] = HIP-event milliseconds of all K-search launches, out[1] = of all
 * K-eval launches, out[2] = K-search launches (turns of the loop that launched none -- a huge topic while KAO-CX / KAO-LP have the GPU
 * -- are not counted), out[3] = restarts, out[4] = algorithmic bytes of those launches (neighbours x (8 RF + 10)),
 * out[5] = neighbours delta-evaluated, out[6] = dynamic LDS per K-search workgroup, out[7] = workgroups per launch.  All zero when
 * the solve was not profiled. */
int kao_last_solve_profile(double out[8]);

#ifdef __cplusplus
}
#endif
#endif /* KAO_H */
