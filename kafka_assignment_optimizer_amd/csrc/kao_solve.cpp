// kao_solve.cpp -- host side of libkao.so, part 3 of 3 (see kao_host.h): the solve loops on top of sessions.
//   kao_solve         one device: K-search launches, K-bound beside them on its own stream, KAO-CX (kao_cycle.hip) for
//                     incumbents the search has stopped improving, stop at the proof
//   kao_solve_multi   several GPUs in one process: topics dealt LPT, or every GPU on every topic with the elites exchanged by
//                     ncclAllReduce(min) / ncclBroadcast on the resident key buffers (librccl is opened on first use)
//   kao_solve_capped  cluster-wide per-broker load caps: Lagrangian prices over independent per-topic solves
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is loaded on first use (kao_solve_multi), see Rccl below
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include "kao_host.h"

namespace {

// The counts of the deterministic schedule (kao_opts.schedule == 0) for a session whose largest topic has `slots` replica
// slots.  Every value is a pure function of the instance and the options -- nothing measured at run time.
struct DetPlan { int bound_iters; int64_t cx_stall_iters, cx_due_iters; int cx_rounds; };
DetPlan det_plan(int64_t slots, int iters_per_launch) {
    DetPlan d;
    // K-bound iterations per launch = about one K-search launch's worth of time, so that neither stream waits for the other
    // (measured on one MI355X, wall-clock schedule with KAO_SOLVE_TRACE=1, profiles/r03_schedule_trace.txt: drifted single
    // topics of 1,000 / 2,000 / 5,000 / 10,000 / 30,000 partitions: K-search launch 1.6 / 4.0 / 4.4 / 7.3 / 8.4 ms with prices, K-bound
    // 29 / 49 / 43 / 48 / 60 us per iteration; the 200-topic config-4 batch: 1.0 ms and 9.5 us).  Interpolated on a log scale
    // of the largest topic's replica slots and rounded down a little: K-bound finishing early costs it some idle time, K-bound
    // finishing late stalls the search.
    // Re-fitted after k_bound_multi (gpurun_out r21, medians of launches without a KAO-CX call, K-bound beside K-search: 1,000 /
    // 2,000 / 5,000 / 10,000 / 30,000 partitions: K-search launch + sync 1.29 / 3.02 / 3.64 / 5.30 / 9.19 ms, K-bound 30.5 / 41.6 /
    // 27.6 / 33.3 / 55.6 us per iteration): the two smallest knots made the search wait 0.4 ms per launch, the larger ones left
    // K-bound idle a quarter of the time.
    static const struct { int64_t slots; int iters; } tab[] = {{512, 128}, {3000, 40}, {6000, 72}, {15000, 120}, {30000, 152}, {90000, 160}};
    const int nt = (int)(sizeof tab / sizeof tab[0]);
    if (slots <= tab[0].slots) d.bound_iters = tab[0].iters;
    else if (slots >= tab[nt - 1].slots) d.bound_iters = tab[nt - 1].iters;
    else {
        int i = 1;
        while (tab[i].slots < slots) ++i;
        // integer interpolation in log2(slots): position of `slots` between the two knots in 1/64 steps
        auto lg64 = [](int64_t v) { int l = 63 - __builtin_clzll((unsigned long long)v); return (int64_t)l * 64 + (((v << 6) >> l) - 64); };
        const int64_t a = lg64(tab[i - 1].slots), b = lg64(tab[i].slots), x = lg64(slots);
        d.bound_iters = (int)(tab[i - 1].iters + (tab[i].iters - tab[i - 1].iters) * (x - a) / std::max<int64_t>(b - a, 1));
    }
    d.bound_iters = std::max(16, d.bound_iters / 8 * 8);
    // KAO-CX pays on a MATURE incumbent: called while K-search still improves it lands in a basin neither comes out of again
    // (24 drifted topics of 1,000-4,000 partitions, 3 s each: first call after 32 launches: 10 proven; after 144: 15).  So a
    // topic counts as stalled after 24 launches without improvement and is otherwise looked at every 144 launches (a call is
    // skipped anyway while the incumbent is the one KAO-CX last ran to a fixpoint on); a call runs at most 12 rounds (6 on
    // topics beyond 30,000 slots, where a round costs as much as several launches).  Test hooks KAO_DET_CX_STALL_L / _DUE_L
    // give both in launches.
    const int64_t it = std::max(iters_per_launch, 1);
    // Beyond a few thousand partitions a launch takes 5-15 ms and KAO-CX is what carries the incumbent (1000 x 30000, 3 s:
    // 231,529 with a call every 6 / 36 launches, 231,159 with 24 / 144), so the counts shrink with the topic.
    // Round 4, beyond 131,072 slots: of a 3-s solve of the drifted 1000 x 100,000 topic KAO-CX's 97 rounds (0.93 s) brought ALL of
    // the 4,275 units gained after the first feasible incumbent, K-search's 126 launches (2 s) none -- there KAO-CX runs after
    // every launch, up to 48 rounds a call (a call ends at the first round that finds nothing).
    const bool huge = slots > 131072;
    // Round 4, up to 16,384 slots: 8 / 48 launches instead of 24 / 144.  Round 3 had found that KAO-CX pays on a MATURE incumbent
    // (first call after 32 launches: 10 of 24 drifted topics proven, after 144: 15); with the two-slot REPLACE scan and the
    // per-rack slack nodes that is no longer so: the whole drifted family (24 topics x solver seeds 3 / 4 / 5, 3 s each) ends
    // 68 of 72 proven in 41 s of wall time with 8 / 48 against 66 of 72 in 58 s with 24 / 144 (GPU call 24; 16 / 96 and 12 / 72
    // on the hard half: 37 and 36 of 42 against 36 and 38).
    const int64_t stall_l = slots <= 16384 ? 8 : (slots <= 32768 ? 12 : (huge ? 1 : 6));
    d.cx_stall_iters = it * env_int("KAO_DET_CX_STALL_L", stall_l);
    d.cx_due_iters = it * env_int("KAO_DET_CX_DUE_L", huge ? 1 : 6 * stall_l);
    d.cx_rounds = (int)env_int("KAO_DET_CX_ROUNDS", slots <= 32768 ? 12 : (huge ? 48 : 6));
    return d;
}

// One whole job on one device: the kao_solve loop, cut into steps so that kao_solve_multi can drive several of them in
// lockstep from one host thread (launches of all devices are enqueued before any of them is waited for).
struct SolveRun {
    kao_session *s = nullptr;
    int n = 0;
    bool has_target = false;
    std::vector<int64_t> target;
    std::vector<uint64_t> keys, prev;
    std::vector<double> t_best;
    std::vector<int64_t> dual_target;
    double t0 = 0, t_last_improve = 0;
    int launches = 0, dual_iters = 0, dual_now = 0;
    // K-bound back-off (round 4, deterministic schedule, topics beyond `bound_rest_slots` replica slots): a K-bound launch beside
    // K-search costs the search more than half its speed there (1000 x 100,000: a K-search launch 6.8 ms alone, 14-19 ms beside
    // K-bound; 1000 x 30,000: 4.0 / 8.4) while the certificate of such a topic stops moving after a second (782,651 from 2.0 s
    // to 10 s with the incumbent still 500 units away).  A topic whose certificate has not moved for kBoundQuiet merged launches
    // is given to K-bound only every kBoundDuty-th time; any improvement of the certificate ends the rest.  Counts only.
    std::vector<int64_t> ub_seen;
    std::vector<int> bound_quiet, bound_turn;
    std::vector<char> bound_ran;
    int64_t bound_rest_slots = 131072;   // (1000 x 30000, 90,000 slots: the rest costs 20-40 units of incumbent and some certificate; 1000 x 100,000: it gains 100-200)
    int bound_quiet_max = 6, bound_duty = 8;
    bool use_prices = true, all_done = false;
    // KAO-CX (kao_cycle.hip): cyclic-exchange improvement of incumbents K-search has stopped improving
    const kao_topic *topics = nullptr;
    std::vector<kao_topic> xt;                    // the session's topics: every caller topic `islands` times
    std::vector<int> origin;                      // session topic -> caller topic
    int n_user = 0;
    bool cx_on = true;
    bool cx_eager = false;                        // test hook KAO_CX_EAGER=1: KAO-CX after every launch, whatever the clock says
    double deadline = 0;
    std::vector<double> t_improved, t_cx;         // per topic: last improvement, last KAO-CX call (seconds from t0)
    std::vector<uint64_t> cx_seen;                // packed key KAO-CX last ran to a fixpoint on
    std::vector<uint16_t> cx_buf;
    std::vector<CycleCtx *> cx_ctx;
    int cx_calls = 0, cx_gains = 0;
    int cx_starts = 0, cx_starts_first = 0, cx_start_rounds = 16, cx_more = 0;   // further KAO-CX starting points per call (further_starts) / in a generation's first call, rounds each, runs so far
    std::vector<int> start_budget, start_near;      // per topic: starts the next call may run; starts of this generation that ended within a unit of the incumbent
    std::vector<std::vector<uint64_t>> cx_started;  // per topic: hashes of the assignments KAO-CX has started from in this generation
    std::vector<int32_t> start_objs;
    std::vector<int> start_order;
    double cx_slice = 0.1;                        // seconds one KAO-CX call may take (wall-clock schedule only)
    // Deterministic schedule (kao_opts.schedule == 0, the default): every decision of the loop is keyed to COUNTS -- K-search
    // launches and iterations, K-bound iterations, KAO-CX rounds -- never to the clock, so the same seed gives the same answer
    // whatever the launch timing (the clock only decides when to stop).  K-bound launches have a fixed length and are merged
    // (waiting for them if need be) after every K-search launch and after every KAO-CX round; KAO-CX is called for a topic that
    // has not improved for `cx_stall_iters` search iterations or has not been through it for `cx_due_iters`, `cx_rounds` rounds
    // per call.
    bool det = true;
    int64_t cx_stall_iters = 0, cx_due_iters = 0;
    int cx_rounds = 0;
    int64_t iters_done = 0;                       // K-search iterations so far (launches x iterations per launch)
    std::vector<int64_t> i_improved, i_cx;        // per topic: iteration count at the last improvement / the last KAO-CX call
    bool trace = false;                           // KAO_SOLVE_TRACE=1: one line per launch on stderr (timings; never read back)
    double t_prev = 0;
    // Generations (deterministic schedule, kao_solve): independent runs of the same topic end 1-2 units apart -- which basin a
    // population converges to is decided early -- so a population that has converged (KAO-CX at a fixpoint of its best, nothing
    // new for `gen_stall_iters`) without a proof is replaced: the incumbent moves to the host, every restart is re-initialised
    // with the generation number in its tie-break hash (kao_session_new_generation), and K-bound, its certificate and its
    // prices carry on, so later generations search under converged prices from their first launch.  The answer is the best
    // incumbent of all generations.
    bool bound_pending = false;                   // a K-bound launch (dual_target, dual_now) waits for the next K-search launch
    bool gens_on = false;
    int generations = 0;
    int64_t gen_stall_iters = 0, gen_start = 0;
    std::vector<uint64_t> dkeys, gprev;           // packed best keys of the CURRENT generation as the device holds them; their record
    std::vector<uint64_t> inc_key;                // best incumbent of the earlier generations (host copy), ~0 = none
    std::vector<std::vector<uint16_t>> inc_assign;
    // KAO-LP (round 5, kao_lp.hip): K-bound's subgradient iteration stalls above the LP value on slack-band and on large topics
    // (450 x 3500: 26336 against 26330 = the incumbent; 1000 x 30000: 231,562 against 231,532; drifted 1000 x 100,000: 782,627
    // against 782,512).  A topic of at least `lp_min_slots` replica slots that the first launch has not closed gets the LP
    // relaxation solved by the interior-point kernels right away (it needs no incumbent; 11-16 iterations = 25-60 ms up to 5,000
    // partitions, where K-bound needs 0.2 s to several seconds or never arrives); a smaller one only after K-bound has had
    // `lp_after_small` merged launches without closing it.  The iterations ride beside the K-search launches on a stream of their
    // own (`lp_per_launch` per launch, no host round trip inside), and when the stop flag is up the row duals become K-bound's
    // multipliers, ONE K-bound iteration evaluates the dual function there in integers (certificate, search prices), and K-bound
    // leaves the topic alone from then on -- it cannot get below the LP value, and beside K-search it costs the search half its
    // speed on large topics.  Counts only: deterministic.
    std::vector<LpCtx *> lp_ctx;
    std::vector<char> lp_state;                   // 0 = not started, 1 = running, 2 = done, 3 = unsupported / failed
    std::vector<int> bound_merges;                // merged K-bound launches per topic
    std::vector<int64_t> lp_tgt;
    std::vector<int> lp_marks, lp_read;           // per topic: marks enqueued / marks read (a mark is read `lp_lag` launches after it was enqueued)
    int lp_lag = 3;
    // Beyond `lp_huge_slots` replica slots (the north-star regime) the pieces do not share the GPU well: K-search there is a grid of
    // dependent random 16-byte reads that saturates the memory system, and beside it the interior point's chain of ~250 small kernels
    // per iteration crawls (drifted 1000 x 100,000: 4 iterations in 250-280 ms beside K-search, 38 ms alone, whatever the stream
    // priority; KAO-CX beside the LP: 20 ms a round instead of 8) -- while K-search itself brings nothing once the topic is feasible
    // (round 4: 0 of 4,275 units; KAO-CX all).  The pieces add up to the same wall time in any order (first feasible incumbent 0.16 s,
    // KAO-CX to its fixpoint 0.8 s, LP 0.53 s), so they run one after the other, the primal side first:
    //   until the first feasible incumbent: K-search;
    //   then KAO-CX to its fixpoint with K-bound beside it (a certificate for whoever stops early), no K-search launches;
    //   then the LP, all its iterations enqueued at once (marks of four), nothing beside it;
    //   then K-search again, under the LP's prices, K-bound retired.
    int64_t lp_huge_slots = 131072;
    std::vector<char> lp_all;                     // per topic: every iteration is enqueued already
    bool huge(int i) const { return (int64_t)topics[i].n_partitions * topics[i].rf > lp_huge_slots; }
    // KAO-LP's primal side (round 5, second half): the LP is solved with PERTURBED costs (kao_lp.hip pert_term) -- small enough that
    // the dual function at its row duals still floors to the LP value (the certificate), large enough that the iterate converges to ONE
    // vertex, which rounds to an assignment (lp_round_assignment).  One solve gives the certificate and, nearly always, the optimum.
    bool lp_round_on = true;      // KAO_LP_ROUND=0: certificate only (the unperturbed LP, as in the first half of round 5)
    double lp_pert_env = -1.0;    // KAO_LP_PERT=<eps>: the perturbation (default min(1e-4, 1.5 / slots))
    double lp_solo_s = 1.0; int64_t lp_solo_slots = 32768;
    int lp_rounded = 0, lp_round_adopted = 0, lp_round_fractional = 0;
    std::vector<int> lp_fan_devs; // kao_solve_multi, KAO_MULTI_LP=shard: the devices ONE sharded LP of a large replicated topic runs on (lp_open_fan); empty: this device alone
    const bool *ext_pause = nullptr;   // ... and the other devices' runs: no K-search launches while the shards of that LP have the GPUs
    int lp_salt0 = 0;             // kao_solve_multi, replicated topics: the device's rank -- every device perturbs the LP with its own salt (a race)
    int lp_round_max_free = 512;  // fractional partitions completed without the incumbent's rows (about 0.1 ms each: 100,000 of a mid-way iterate took 8 s)
    std::vector<char> lp_try, lp_certified;   // per topic: LP solves finished; the LP's certificate is in place (K-bound leaves the topic alone)
    double lp_tol = 1e-10;        // stopping tolerance of the perturbed solve (KAO_LP_TOL)
    int lp_ahead = 4;             // huge topics: marks (of four iterations) kept enqueued ahead of the one being waited for
    int lp_max_tries = 3;         // a rounded iterate that is not the optimum: up to two more solves, larger perturbation, other salts, primal side only
    bool lp_retry_test = false;   // test hook KAO_LP_RETRY_TEST=1: the first rounded iterate is discarded
    std::vector<uint8_t> lp_q;
    std::vector<int32_t> lp_zq;
    std::vector<uint16_t> lp_buf, lp_fb;
    double lp_pert_of(int i) const {
        if (!lp_round_on) return 0.0;
        if (lp_pert_env >= 0) return lp_pert_env;
        return std::min(1e-4, 1.5 / ((double)topics[i].n_partitions * topics[i].rf));
    }
    bool lp_possible(int i) const { return lp_on && !has_target && dual_iters > 0 && s->dual_ok[(size_t)i] && lp_state[(size_t)i] < 2; }
    // the LP alone on the GPU, before any K-search launch: huge topics when the limit leaves room for it (lp_fits), topics from
    // lp_solo_slots replica slots (1000 x 30000: 0.56 s alone, 1.0 s two iterations per K-search launch) when it is at least a second
    // (a limit is an input, not the clock: the schedule stays count-keyed)
    bool solo(int i) const { return !huge(i) && (int64_t)topics[i].n_partitions * topics[i].rf >= lp_solo_slots; }
    bool only_open(int i) const {   // no other topic still waits for the search (a paused K-search would starve it)
        for (int j = 0; j < n; ++j) if (j != i && !topic_done(j)) return false;
        return true;
    }
    // Predicted seconds of ONE perturbed interior-point solve of topic i alone on the device, from counts (the choice of
    // algorithm was keyed on fixed limits, 1.5 / 1.3 s, so a 1-second caller never got the LP).  An iteration costs lp_ms_base +
    // lp_ms_tile per 64-row tile of the Schur complement (3R + 2B rows: the Cholesky and the triangular solves walk the tiles one after
    // the other) + lp_ms_kpart per 1,000 partitions (everything else streams the partitions); the perturbed solve takes 35-55
    // iterations at tolerance 1e-10 on drifted topics of 30,000-300,000 partitions (lp_iters_est; 105-150 before the centering exponent 10, the
    // step fraction and the starting point's floor, docs/notes_r06.md sections 23-25), plus lp_s_fixed + lp_s_kpart per 1,000 partitions for the context, the
    // starting point, the read-back and the rounding (0.12 s at 100,000 partitions).  Constants measured on one MI355X (round 6, profiles/r06_*); a limit is an input,
    // not the clock: the schedule stays count-keyed.
    double lp_ms_base = 0.50, lp_ms_tile = 0.05, lp_ms_kpart = 0.020, lp_iters_est = 60.0, lp_s_fixed = 0.06, lp_s_kpart = 0.0006, lp_fit = 0.8;
    // beyond 20 racks both grow (1000 x 100,000 at 30 / 40 / 50 racks: 4.9 / 5.9 / 6.7 ms an iteration against 4.0; 74 iterations at 40 racks against 66 at 20): the
    // per-partition rack work of the eliminations and of the Schur rows, and a slower approach to the vertex
    double lp_ms_kpart_rack = 0.0009, lp_iters_rack = 0.5;
    double lp_reserve_s = 0.2;    // an LP that runs before there is any incumbent is given up this long before the deadline: K-search needs ~0.16 s to a first feasible plan at 100,000 partitions
    double lp_wait_until(int i) const { return feasible(i) ? deadline : deadline - lp_reserve_s; }
    double lp_est_s(int i) const {
        const kao_topic &t = topics[i];
        const int nt = (3 * t.n_racks + 2 * t.n_brokers + 63) / 64;
        const double xr = std::max(0, t.n_racks - 20);
        return lp_s_fixed + lp_s_kpart * t.n_partitions / 1000.0 + 1e-3 * (lp_iters_est + lp_iters_rack * xr) * (lp_ms_base + lp_ms_tile * nt + (lp_ms_kpart + lp_ms_kpart_rack * xr) * t.n_partitions / 1000.0);
    }
    bool lp_fits(int i, double extra_s = 0.0) const { return lp_est_s(i) + extra_s <= lp_fit * (deadline - t0); }
    bool lp_alone(int i) const {
        if (!lp_round_on) return false;
        return (huge(i) && lp_fits(i)) || (solo(i) && deadline - t0 >= lp_solo_s && only_open(i));
    }
    // a huge topic whose limit leaves no room for its LP beside the incumbent: the first LP starts once KAO-CX has run the incumbent to a
    // fixpoint, so KAO-CX must not wait for that LP (both would wait while the search is paused, until the deadline)
    bool lp_waits_for_cx(int i) const {
        return huge(i) && !lp_alone(i) && !(lp_round_on && lp_fits(i, 0.2)) && cx_on && cycle_supported(&topics[i]);
    }
    // a huge topic between its first feasible incumbent and the end of its LP -- from the start when the limit leaves room for the LP alone
    bool pause_wanted(int i) const { return lp_possible(i) && ((huge(i) && feasible(i)) || lp_alone(i)); }
    static constexpr int kFirstShortIters = 32;
    int iters_last = 0;           // iterations of the launch just enqueued
    bool first_launch_short() const {
        if (s->opts.max_launches > 0 || !lp_on || has_target || dual_iters <= 0) return false;
        // (this does run: at turn 0 every key is still 0, which feasible() reads as feasible at objective kObjCap >= ub, so topic_done holds and search_paused() is false)
        for (int i = 0; i < n; ++i)
            if (!(huge(i) && lp_alone(i) && s->dual_ok[(size_t)i] && !s->topic_infeasible[(size_t)i])) return false;
        return n > 0;
    }
    bool search_paused() const {
        //  never when the caller counts K-search launches (max_launches: it gets them), and never while some other open topic
        // still needs the search: a pause is for solves whose every open topic is waiting for its LP
        if (s->opts.max_launches > 0) return false;
        if (ext_pause && *ext_pause) return true;
        bool any = false;
        for (int i = 0; i < n; ++i) {
            if (topic_done(i)) continue;
            if (!pause_wanted(i)) return false;
            any = true;
        }
        return any;
    }
    int lp_on = 1, lp_per_launch = 2, lp_per_turn_max = 48, lp_max_running = 8, lp_solves = 0, lp_iters = 0;
    int64_t lp_mid_slots = 8192;   // from here on the LP is what proves a drifted topic: more iterations per turn, KAO-CX behind it
    int64_t lp_min_slots = 2048;
    int lp_after_small = 48;

    ~SolveRun() { for (CycleCtx *c : cx_ctx) cycle_close(c); for (LpCtx *c : lp_ctx) if (c) { lp_abort(c); lp_close(c); } if (s) kao_session_destroy(s); }

    // `so` is the caller's options with kao_solve's defaults applied; the session is created on the calling thread's device
    int begin(const kao_topic *user_topics, int n_topics, const kao_opts &so, const int64_t *tgt, double t_start, bool allow_islands = false, bool allow_gens = false) {
        t0 = t_start;
        n_user = n_topics;
        // Islands (kao_opts.islands > 1, off by default): every topic is searched as several independent copies (own seed,
        // own restarts, own elite, own K-bound trajectory and prices, own KAO-CX) sharing one copy's restart budget;
        // certificates are shared, the best copy answers.  Measured on the drifted 300 x 2000 topic (4 islands, 4 seeds,
        // 8 s): 14825 / 14825 / 14824 / 14822 against 14825 / 14826 (proven) / ... without -- no gain, so not the default.
        int k = 1;
        if (allow_islands && user_topics && n_topics >= 1 && so.restarts <= 0 && so.islands > 1) k = std::min(so.islands, 8);
        xt.clear(); origin.clear();
        for (int i = 0; i < n_topics; ++i)
            for (int c = 0; c < k; ++c) { xt.push_back(user_topics[i]); origin.push_back(i); }
        const kao_topic *topics = xt.data();
        kao_opts so_x = so;
        if (k > 1) {   // the islands share what one copy would have got: same work per launch, k basins
            int64_t slots = 1;
            for (int i = 0; i < n_topics; ++i) slots = std::max<int64_t>(slots, (int64_t)user_topics[i].n_partitions * std::max(user_topics[i].rf, 1));
            (void)require_init();
            const int cu = std::max(num_cu(cur_device()), 1);
            int r = std::min(std::max((cu * 32 / n_topics) / kWaves * kWaves, 8), 8192);
            r = std::min<int>(r, (int)std::max<int64_t>(cu, (((int64_t)1 << 22) / slots) / kWaves * kWaves));
            so_x.restarts = std::max((r / k) / kWaves * kWaves, 2 * kWaves);
        }
        if (k == 1 && so.restarts <= 0 && user_topics) {
            // Topics that live in HBM (not even the working assignment of one restart fits LDS): a session on its own fills the chip with 4
            // restarts per compute unit (kao_session_create); the solve keeps TWO per compute unit.  Round 4 kept one -- beside K-bound depth
            // paid, breadth did not (256 against 1024 restarts: 1000 x 30000 231,530 / 231,522 against 231,511 / 231,522) -- but since round 5
            // K-bound retires as soon as KAO-LP has certified the topic, and a launch of 512 restarts takes hardly longer than one of 256
            // (1000 x 30000, 4 s, seeds 3 / 4 / 5: 231,527 / 231,516 / 231,532 PROVEN with 512; 231,522 / 231,516 / 231,518 with 256; 231,511 /
            // 231,516 / 231,518 with 1,024; 500 x 10000: 76,351 / 76,352 / 76,354 proven against 76,345 / 76,352 / 76,351; GPU call 24).
            int64_t slots = 1;
            bool hbm = false;
            for (int i = 0; i < n_topics; ++i) {
                const kao_topic &t = user_topics[i];
                slots = std::max<int64_t>(slots, (int64_t)t.n_partitions * std::max(t.rf, 1));
                const int nw = (t.rf > kRFP || t.rf_cur > kRFP) ? 2 * kRFP : kRFP;
                hbm = hbm || (int64_t)t.n_partitions * nw * 4 + 8 * 1024 > 160 * 1024;
            }
            if (hbm && !require_init()) {
                // never more than the session's own automatic count (with many topics beside a large one the override
                // multiplied the wavefronts per launch: 100 topics of 11,000 partitions went from 80 to 256 restarts each)
                const int cu = std::max(num_cu(cur_device()), 1);
                const int64_t auto_r = std::min(std::max((cu * 32 / std::max(n_topics, 1)) / kWaves * kWaves, 8), 8192);
                so_x.restarts = (int)std::min<int64_t>(auto_r, std::max<int64_t>(2 * cu, (((int64_t)1 << 22) / slots) / kWaves * kWaves));
            }
        }
        n = n_topics = (int)xt.size();
        int rc = kao_session_create(topics, n_topics, &so_x, &s);
        if (rc) return rc;
        has_target = tgt != nullptr;
        if (tgt) { target.resize((size_t)n); for (int i = 0; i < n; ++i) target[(size_t)i] = tgt[origin[(size_t)i]]; }
        keys.assign((size_t)n, 0); prev.assign((size_t)n, ~0ull); t_best.assign((size_t)n, 0.0); dual_target.assign((size_t)n, -1);
        ub_seen.assign((size_t)n, INT64_MAX); bound_quiet.assign((size_t)n, 0); bound_turn.assign((size_t)n, 0); bound_ran.assign((size_t)n, 0);
        dkeys.assign((size_t)n, ~0ull); gprev.assign((size_t)n, ~0ull); inc_key.assign((size_t)n, ~0ull); inc_assign.assign((size_t)n, {});
        this->topics = topics;
        t_improved.assign((size_t)n, 0.0); t_cx.assign((size_t)n, 0.0); cx_seen.assign((size_t)n, ~0ull);
        cx_started.assign((size_t)n, {});
        lp_ctx.assign((size_t)n, nullptr); lp_marks.assign((size_t)n, 0); lp_read.assign((size_t)n, 0); lp_all.assign((size_t)n, 0); lp_state.assign((size_t)n, 0); lp_try.assign((size_t)n, 0); lp_certified.assign((size_t)n, 0); bound_merges.assign((size_t)n, 0); lp_tgt.assign((size_t)n, -1);
        {   // test / experiment hooks: KAO_LP=0 switches KAO-LP off, KAO_LP_AFTER / KAO_LP_PER_LAUNCH / KAO_LP_MIN_SLOTS override the counts
            lp_on = (int)env_int("KAO_LP", 1);
            lp_after_small = (int)env_int("KAO_LP_AFTER", lp_after_small);
            lp_per_launch = (int)std::max<int64_t>(1, env_int("KAO_LP_PER_LAUNCH", lp_per_launch));
            lp_min_slots = env_int("KAO_LP_MIN_SLOTS", lp_min_slots);
            lp_round_on = env_int("KAO_LP_ROUND", 1) != 0;
            lp_max_tries = env_int("KAO_LP_TRIES", 3);
            lp_max_running = (int)std::max<int64_t>(1, env_int("KAO_LP_MAX_RUNNING", lp_max_running));
            lp_tol = env_real("KAO_LP_TOL", lp_tol);
            lp_retry_test = env_int("KAO_LP_RETRY_TEST", 0) != 0;
            lp_pert_env = env_real("KAO_LP_PERT", lp_pert_env);
            lp_solo_s = env_real("KAO_LP_SOLO_S", lp_solo_s);
            lp_solo_slots = env_int("KAO_LP_SOLO_SLOTS", 32768);
        }
        cx_on = so.use_cycles >= 0;
        cx_eager = env_int("KAO_CX_EAGER", 0) != 0;
        cx_ctx.assign((size_t)n, nullptr);
        cx_slice = std::max(0.1, 0.1 * (so.time_limit_s > 0 ? so.time_limit_s : 10.0));
        deadline = t_start + (so.time_limit_s > 0 ? so.time_limit_s : 10.0);
        const kao_opts &o = s->opts;
        dual_iters = o.dual_iters < 0 ? 0 : (o.dual_iters == 0 ? 128 : o.dual_iters);
        dual_now = dual_iters;
        det = so.schedule == 0;
        s->bound_no_wait = det;   // K-bound launches start at points where no K-search launch reads the price half they write
        i_improved.assign((size_t)n, 0); i_cx.assign((size_t)n, 0);
        {   // the counts of the deterministic schedule, from the size of the largest topic (constants measured on one MI355X so
            // that a K-bound launch takes about as long as a K-search launch and KAO-CX gets about the share of the wall clock
            // the time slices of the wall-clock schedule gave it).  Test / tuning hooks: KAO_DET_*.
            int64_t slots = 1;
            for (int i = 0; i < n; ++i) slots = std::max<int64_t>(slots, (int64_t)topics[i].n_partitions * std::max(topics[i].rf, 1));
            const DetPlan dp = det_plan(slots, o.iters_per_launch);
            if (det && o.dual_iters == 0) dual_now = dual_iters = dp.bound_iters;
            cx_stall_iters = dp.cx_stall_iters; cx_due_iters = dp.cx_due_iters; cx_rounds = dp.cx_rounds;
            if (det) { dual_now = dual_iters = dual_iters > 0 ? (int)env_int("KAO_DET_BOUND_ITERS", dual_iters) : 0; }
            cx_stall_iters = env_int("KAO_DET_CX_STALL", cx_stall_iters); cx_due_iters = env_int("KAO_DET_CX_DUE", cx_due_iters);
            cx_rounds = (int)env_int("KAO_DET_CX_ROUNDS", cx_rounds);
            // further KAO-CX starting points per call (further_starts): where a round is cheap (closures of (B + 1)^2 entries, <= 512
            // realisations of P rows) eight more descents cost about as much as the launches between two calls
            cx_starts = (int)env_int("KAO_DET_CX_STARTS", slots <= 16384 ? 8 : 0);
            cx_starts_first = (int)env_int("KAO_DET_CX_STARTS_FIRST", 2 * cx_starts);
            cx_start_rounds = (int)env_int("KAO_DET_CX_START_ROUNDS", 16);
            start_budget.assign((size_t)n, cx_starts_first); start_near.assign((size_t)n, 0);
        }
        gens_on = allow_gens && det && cx_on && !has_target;
        if (env_int("KAO_DET_GEN", 1) == 0) gens_on = false;
        {   // a new population needs time in proportion to the topic to catch up with the one it replaces (1000 x 30000, 3 s: a
            // restart after 32 quiet launches cost 100 units): the patience grows with the largest topic's replica slots
            int64_t slots = 1;
            for (int i = 0; i < n; ++i) slots = std::max<int64_t>(slots, (int64_t)topics[i].n_partitions * std::max(topics[i].rf, 1));
            gen_stall_iters = env_int("KAO_DET_GEN_STALL_L", 32 * std::max<int64_t>(1, slots / 8192)) * (int64_t)std::max(o.iters_per_launch, 1);
        }
        trace = env_int("KAO_SOLVE_TRACE", 0) != 0;
        t_prev = t_start;
        use_prices = so.use_prices >= 0;
        return KAO_OK;
    }
    // asynchronous.  Deterministic schedule: the K-bound launch decided after the previous K-search launch is enqueued only
    // now, behind the new K-search launch -- enqueueing up to 176 step kernels takes the host about a millisecond, which
    // the search stream no longer spends idle
    bool stepped = false;     // the last turn launched K-search (a paused turn does not count as a launch)
    int turns = 0;
    double t_turn = 0, turn_s = 0;   // when the previous turn began; how long the turns take (smoothed)
    // Interior-point iterations enqueued beside one launch.  Two (lp_per_launch) suit launches of a few milliseconds; twenty topics of 5,000
    // partitions or ten of 12,000 turn every ~0.2 s, and at two iterations a turn an LP of a hundred iterations took fifty turns (round 6,
    // tools/r6_scenarios2.py: 5 of 20 topics proven in 10 s, four LP solves finished).  So the count follows the clock: what the LP's own
    // estimate says fits one turn, shared by the solves in flight; the deterministic schedule goes by the topic's size (8 iterations a turn from
    // lp_mid_slots replica slots on, 16 from 32,768), up to eight solves in flight (2 / 4 / 8 / 16: 2.8 / 2.2 / 1.9 / 1.7 s on twenty topics of 5,000 partitions), and KAO-CX leaves such a topic alone until its LP has spoken:
    // the one turn in which every stalled topic got its KAO-CX calls was 8.5 s of that solve, with the LP streams idle.
    int lp_iters_this_turn(int i, int running) const {
        if (det || turn_s <= 0) {   // counts: a pure function of the topic's size (a launch over topics of 8,192+ slots takes tens of milliseconds)
            const int64_t slots = (int64_t)topics[i].n_partitions * topics[i].rf;
            return slots >= 32768 ? std::max(lp_per_launch, 16) : (slots >= lp_mid_slots ? std::max(lp_per_launch, 8) : lp_per_launch);
        }
        const kao_topic &t = topics[i];
        const int nt = (3 * t.n_racks + 2 * t.n_brokers + 63) / 64;
        const double xr = std::max(0, t.n_racks - 20);
        const double ms = lp_ms_base + lp_ms_tile * nt + (lp_ms_kpart + lp_ms_kpart_rack * xr) * t.n_partitions / 1000.0;
        return (int)std::min<double>(lp_per_turn_max, std::max<double>(lp_per_launch, turn_s * 1e3 / (ms * std::max(1, running))));
    }
    int lp_lag_now() const { return (!det && turn_s > 0.02) ? 1 : lp_lag; }   // (a mark is a turn's worth of iterations then: read a turn later)
    int launch() {
        int rc = KAO_OK;
        const double tn = now_s();
        if (t_turn > 0) turn_s = turn_s > 0 ? 0.5 * turn_s + 0.5 * (tn - t_turn) : tn - t_turn;
        t_turn = tn;
        stepped = !search_paused();
        if (stepped) {
            // The first launch of a solve whose every topic gets its LP without waiting for an incumbent (huge, and the LP's predicted time fits
            // the limit) is K-init + kFirstShortIters iterations instead of a whole launch: on a drifted 100,000-partition topic the 512
            // iterations (17 ms) end without a feasible plan anyway and the LP's kernels find no free compute unit until they have drained; a
            // balanced start is proven by K-init's plan either way.  A count, not the clock.
            const int ipl = s->opts.iters_per_launch;
            if (turns == 0 && first_launch_short()) s->opts.iters_per_launch = std::min(ipl, kFirstShortIters);
            rc = kao_session_step(s);
            iters_last = s->opts.iters_per_launch;
            s->opts.iters_per_launch = ipl;
        }
        if (!rc && bound_pending) { bound_pending = false; rc = kao_session_bound_step(s, dual_target.data(), dual_now); }
        int running = 0;
        for (int i = 0; i < n; ++i) running += lp_state[(size_t)i] == 1 && !lp_all[(size_t)i];
        for (int i = 0; i < n && !rc; ++i)
            if (lp_state[(size_t)i] == 1 && !lp_all[(size_t)i]) rc = lp_enqueue_mark(lp_ctx[(size_t)i], lp_iters_this_turn(i, running), lp_marks[(size_t)i]++);   // interior-point iterations beside the launch
        return rc;
    }
    // KAO-LP: start the LP of topics K-bound has not closed, collect the ones whose stop flag is up
    int service_lp(bool final_call = false) {
        if (!lp_on || has_target || dual_iters <= 0) return KAO_OK;
        const double tsl0 = now_s();
        struct Tr { bool on; double t0; int l; ~Tr() { if (on && now_s() - t0 > 2e-3) std::fprintf(stderr, "[kao-solve]   service_lp took %.3f ms at launch %d\n", (now_s() - t0) * 1e3, l); } } tr_{trace, tsl0, launches};
        int rc, running = 0;
        for (int i = 0; i < n; ++i) running += lp_state[(size_t)i] == 1;
        for (int i = 0; i < n; ++i) {
            if (lp_state[(size_t)i] != 1) continue;
            int st = 0, it = 0;
            // the mark of `lp_lag` launches ago (the interior-point stream runs on while the host goes about K-search, K-bound and KAO-CX:
            // it is hardly ever waited for); at the end of the solve the newest one
            if (final_call) {   // the newest mark of an LP that rides beside the launches; of one enqueued as a whole only the next (a bounded wait)
                const int m = lp_all[(size_t)i] ? lp_read[(size_t)i] : lp_marks[(size_t)i] - 1;
                if (m >= 0 && m < lp_marks[(size_t)i] && (rc = lp_poll_mark(lp_ctx[(size_t)i], m, &st, &it, deadline))) return rc;
                if (st == 4) st = 0;   // aborted at the deadline: a mid-way iterate, not a result
                if (!st) lp_abort(lp_ctx[(size_t)i]);
            } else if (lp_read[(size_t)i] < lp_marks[(size_t)i] && lp_marks[(size_t)i] - lp_read[(size_t)i] > (lp_all[(size_t)i] ? 0 : lp_lag_now())) {
                const double tp0 = now_s();
                if ((rc = lp_poll_mark(lp_ctx[(size_t)i], lp_read[(size_t)i]++, &st, &it, lp_all[(size_t)i] ? lp_wait_until(i) : 0.0))) return rc;   // (a huge topic's LP is waited for: the wait ends at the deadline)
                if (st == 4) {   // aborted at the deadline: no certificate, no rounding of a mid-way iterate; the main loop ends on the clock
                    lp_close(lp_ctx[(size_t)i]); lp_ctx[(size_t)i] = nullptr; lp_state[(size_t)i] = 3; --running;
                    continue;
                }
                if (lp_all[(size_t)i] && !st && lp_marks[(size_t)i] < 64 && (rc = lp_enqueue_mark(lp_ctx[(size_t)i], 4, lp_marks[(size_t)i]++))) return rc;
                if (trace) std::fprintf(stderr, "[kao-solve]   KAO-LP topic %d: mark %d of %d read in %.3f ms: %d iterations, stop %d\n", i, lp_read[(size_t)i] - 1, lp_marks[(size_t)i], (now_s() - tp0) * 1e3, it, st);
            }
            const bool open = feasible(i) ? objective(i) < s->ub[(size_t)i] : true;
            if (!st && open && !final_call) continue;
            if (!st || !open) { lp_abort(lp_ctx[(size_t)i]); lp_close(lp_ctx[(size_t)i]); lp_ctx[(size_t)i] = nullptr; lp_state[(size_t)i] = open ? 0 : 2; --running; continue; }
            // the row duals as K-bound's multipliers; one K-bound iteration evaluates the dual function there in integers
            const kao_topic &t = topics[i];
            std::vector<int32_t> mult(2 * (size_t)t.n_brokers + (size_t)t.n_racks);
            double st8[8];
            const double tf0 = now_s();
            rc = lp_finish(lp_ctx[(size_t)i], mult.data(), st8, nullptr);
            const double tf1 = now_s();
            bool have_primal = false;
            if (!rc && lp_round_on && st8[3] != 3.0) {   // the quantised iterate (not of a stalled solve: its last iterate is not finite)
                lp_q.resize((size_t)(2 * t.rf_cur + 2 * t.n_racks) * t.n_partitions); lp_zq.resize(2 * (size_t)t.n_brokers);
                have_primal = lp_primal(lp_ctx[(size_t)i], lp_q.data(), lp_zq.data()) == KAO_OK;
            }
            const double tf2 = now_s();
            lp_close(lp_ctx[(size_t)i]); lp_ctx[(size_t)i] = nullptr; --running;
            if (trace) std::fprintf(stderr, "[kao-solve]   KAO-LP topic %d: lp_finish %.3f ms, lp_primal %.3f ms, lp_close %.3f ms\n", i, (tf1 - tf0) * 1e3, (tf2 - tf1) * 1e3, (now_s() - tf2) * 1e3);
            if (rc) { lp_state[(size_t)i] = 3; continue; }
            lp_iters += it; ++lp_solves;
            const bool primal_only = lp_try[(size_t)i]++ > 0;   // a retry: the certificate and the prices of the first solve stay
            if (primal_only) {
                lp_state[(size_t)i] = 2;
                if (trace) std::fprintf(stderr, "[kao-solve]   KAO-LP topic %d: solve %d (primal side only): %d iterations, launch %d\n", i, (int)lp_try[(size_t)i], it, launches);
                if (have_primal && (rc = lp_round_and_adopt(i))) return rc;
                if (!topic_done(i) && lp_try[(size_t)i] < (huge(i) ? std::min(2, lp_max_tries) : lp_max_tries)) lp_state[(size_t)i] = 0;
                continue;
            }
            if (s->bound_inflight && (rc = kao_session_bounds(s, nullptr, nullptr, nullptr))) return rc;
            if ((rc = kao_session_set_dual_state(s, i, mult.data(), mult.data() + t.n_brokers, mult.data() + 2 * (size_t)t.n_brokers))) return rc;
            std::fill(lp_tgt.begin(), lp_tgt.end(), -1);
            lp_tgt[(size_t)i] = feasible(i) ? objective(i) : 0;
            if ((rc = kao_session_bound_step(s, lp_tgt.data(), 1)) || (rc = kao_session_bounds(s, nullptr, nullptr, nullptr))) return rc;
            share_bounds();
            if (use_prices && (rc = kao_session_adopt_prices(s))) return rc;
            lp_state[(size_t)i] = 2; lp_certified[(size_t)i] = 1;
            if (trace) std::fprintf(stderr, "[kao-solve]   KAO-LP topic %d: %d iterations, LP value %.4f, certificate %lld, launch %d\n", i, it, st8[2], (long long)s->ub[(size_t)i], launches);
            if (have_primal && !(lp_retry_test && lp_try[(size_t)i] == 1) && (rc = lp_round_and_adopt(i))) return rc;
            if (lp_round_on && !topic_done(i) && lp_try[(size_t)i] < (huge(i) ? std::min(2, lp_max_tries) : lp_max_tries)) lp_state[(size_t)i] = 0;   // not the optimum: once more, primal side only (huge topics: once; the search waits meanwhile)
        }
        if (final_call) return KAO_OK;
        // largest open topics first, at most `lp_max_running` at a time
        for (;;) {
            if (running >= lp_max_running || now_s() >= deadline) break;
            int best = -1; int64_t best_slots = 0;
            for (int i = 0; i < n; ++i) {
                if (lp_state[(size_t)i] != 0 || !s->dual_ok[(size_t)i] || s->topic_infeasible[(size_t)i] || (feasible(i) && objective(i) >= s->ub[(size_t)i])) continue;
                if (huge(i)) {   // ... once KAO-CX has run the incumbent to a fixpoint (or cannot run) -- or, when the time
                    // limit leaves room for it (a limit is an input, not the clock), straight after the first feasible incumbent: its
                    // primal side makes the fixpoint unnecessary
                    if (!lp_alone(i) && (!feasible(i) || (lp_waits_for_cx(i) && (dkeys[(size_t)i] >> 20) != (cx_seen[(size_t)i] >> 20)))) continue;
                }
                const int64_t slots = (int64_t)topics[i].n_partitions * topics[i].rf;
                if (slots < lp_min_slots && !lp_try[(size_t)i] && (!feasible(i) || bound_merges[(size_t)i] < lp_after_small)) continue;
                if (slots > best_slots) { best = i; best_slots = slots; }
            }
            if (best < 0) break;
            LpCtx *c = nullptr;
            if (!lp_fan_devs.empty() && (huge(best) || solo(best))) rc = lp_open_fan(&topics[best], lp_fan_devs.data(), (int)lp_fan_devs.size(), &c);   // one LP over all devices
            else rc = lp_open(&topics[best], &c);
            if (rc == KAO_ERR_UNSUPPORTED || rc == KAO_ERR_NOMEM) { lp_state[(size_t)best] = 3; continue; }
            if (rc) return rc;
            const bool retry = lp_try[(size_t)best] > 0;   // primal side only: the larger perturbation of kao_lp_round, another salt
            const double pert = retry ? lp_default_pert(&topics[best]) : lp_pert_of(best);
            if ((rc = lp_begin(c, retry ? 1e-8 : (pert > 0 ? lp_tol : 1e-7), pert > 0 ? 200 : 120, pert, (uint32_t)(lp_try[(size_t)best] + 16 * lp_salt0)))) { lp_close(c); return rc; }
            lp_ctx[(size_t)best] = c; lp_state[(size_t)best] = 1; lp_marks[(size_t)best] = lp_read[(size_t)best] = 0; lp_all[(size_t)best] = 0; ++running;
            if (huge(best) || lp_alone(best)) {   // alone on the GPU and driven from here: a few marks of four iterations ahead, one more whenever one is read (iterations
                // behind the stop flag are no-ops, but ~250 empty kernels each: enqueueing the whole solve left 0.1 s of them behind an early stop)
                for (int m = 0; m < lp_ahead; ++m) if ((rc = lp_enqueue_mark(c, 4, lp_marks[(size_t)best]++))) return rc;
                lp_all[(size_t)best] = 1;
            }
        }
        all_done = check_done();
        return KAO_OK;
    }
    // the quantised iterate in lp_q / lp_zq -> an assignment (fractional partitions keep the incumbent's rows), scored exactly; a feasible
    // one that beats the incumbent becomes the incumbent and the elite (as a KAO-CX result does)
    int lp_round_and_adopt(int i) {
        const kao_topic &t = topics[i];
        const size_t slots = (size_t)t.n_partitions * t.rf;
        const double tr0 = now_s();
        lp_buf.resize(slots);
        const uint16_t *fb = nullptr;
        int rc;
        if (gfeasible(i)) { lp_fb.resize(slots); if ((rc = session_topic_best(s, i, lp_fb.data()))) return rc; fb = lp_fb.data(); }
        // fractional partitions take their heaviest options first (they follow the LP's mass and the inflows that are left); only when
        // that breaks a band row do they keep the incumbent's rows instead (an incumbent far from the LP's vertex fits the inflows worse:
        // drifted 1000 x 100,000, 9 fractional partitions: optimal with the options, 5 violations with the rows of the first feasible incumbent)
        int32_t rep[4] = {0, 0, 0, 0};
        int64_t obj = 0;
        int32_t viol[8] = {0};
        if (now_s() >= deadline) return KAO_OK;
        if ((rc = lp_round_assignment(&t, lp_q.data(), lp_zq.data(), nullptr, lp_buf.data(), rep, lp_round_max_free))) return rc;
        if (rep[3] < 0) {   // far from a vertex: too many fractional partitions to complete freely -- the incumbent's rows, or nothing
            if (!fb) { ++lp_rounded; lp_round_fractional += rep[0]; return KAO_OK; }
            if ((rc = lp_round_assignment(&t, lp_q.data(), lp_zq.data(), fb, lp_buf.data(), rep))) return rc;
        }
        if ((rc = kao_evaluate(&t, lp_buf.data(), &obj, viol))) return rc;
        if (viol[0] != 0 && fb && rep[0] > 0 && rep[3] == 0) {
            if ((rc = lp_round_assignment(&t, lp_q.data(), lp_zq.data(), fb, lp_buf.data(), rep)) || (rc = kao_evaluate(&t, lp_buf.data(), &obj, viol))) return rc;
        }
        ++lp_rounded; lp_round_fractional += rep[0];
        const bool better = viol[0] == 0 && (!gfeasible(i) || obj > gobjective(i));
        if (trace) std::fprintf(stderr, "[kao-solve]   KAO-LP topic %d: rounded iterate: objective %lld violations %d (%d fractional partitions, %d beyond an inflow, %d rows from the incumbent) in %.3f ms%s\n",
                                i, (long long)obj, viol[0], rep[0], rep[1] + rep[2], rep[3], (now_s() - tr0) * 1e3, better ? ": adopted" : "");
        if (!better) return KAO_OK;
        uint64_t key = 0;
        if ((rc = session_adopt_external(s, i, lp_buf.data(), obj, &key))) return rc;
        const double t2 = now_s() - t0;
        dkeys[(size_t)i] = gprev[(size_t)i] = key;
        t_improved[(size_t)i] = t2;
        i_improved[(size_t)i] = iters_done;
        if (key < keys[(size_t)i]) { keys[(size_t)i] = prev[(size_t)i] = key; t_best[(size_t)i] = t_last_improve = t2; }
        ++lp_round_adopted;
        // a rounded iterate that is feasible but a few units under the certificate (a half-integral vertex: the completion of its
        // fractional partitions is feasible, not optimal) is local work for KAO-CX -- a descent from it costs a few rounds, another
        // interior-point solve a second at 100,000 partitions
        if (cx_on && !has_target && !topic_done(i) && cycle_supported(&t) && now_s() < deadline) {
            cx_buf.assign(lp_buf.begin(), lp_buf.end());
            if (!cx_ctx[(size_t)i] && !(cx_ctx[(size_t)i] = cycle_open(&topics[i], &rc))) return rc;
            if ((rc = cycle_start(i, gobjective(i), det ? 2 * cx_rounds : 0, true))) return rc;
        }
        return KAO_OK;
    }
    // keys = the best over all generations (what "done", the K-bound targets and the answer go by); dkeys = this generation's
    bool feasible(int i) const { return (keys[(size_t)i] >> 44) == 0; }
    int64_t objective(int i) const { return (int64_t)kObjCap - (int64_t)((keys[(size_t)i] >> 20) & 0xFFFFFF); }
    bool gfeasible(int i) const { return (dkeys[(size_t)i] >> 44) == 0; }
    int64_t gobjective(int i) const { return (int64_t)kObjCap - (int64_t)((dkeys[(size_t)i] >> 20) & 0xFFFFFF); }
    bool topic_done(int i) const {
        if (s->topic_infeasible[(size_t)i]) return true;  // proven infeasible: nothing to wait for
        const int64_t goal = has_target ? target[(size_t)i] : s->ub[(size_t)i];
        return feasible(i) && objective(i) >= goal;
    }
    bool check_done() const {   // every caller topic has one island that is done
        for (int i = 0; i < n;) {
            bool any = false;
            int j = i;
            for (; j < n && origin[(size_t)j] == origin[(size_t)i]; ++j) any = any || topic_done(j);
            if (!any) return false;
            i = j;
        }
        return true;
    }
    void share_bounds() {       // a certificate of any island holds for its caller topic
        for (int i = 0; i < n;) {
            int64_t ub = INT64_MAX;
            int j = i;
            for (; j < n && origin[(size_t)j] == origin[(size_t)i]; ++j) ub = std::min(ub, s->ub[(size_t)j]);
            for (int q = i; q < j; ++q) s->ub[(size_t)q] = ub;
            i = j;
        }
    }
    // waits for the launch, books improvements, merges a finished K-bound launch and starts the next one
    int after_launch() {
        int rc = kao_session_best_keys(s, dkeys.data());
        if (rc) return rc;
        ++turns;
        if (stepped) { ++launches; iters_done += iters_last; }
        const double t = now_s() - t0;
        for (int i = 0; i < n; ++i) {
            if (dkeys[(size_t)i] < gprev[(size_t)i]) { gprev[(size_t)i] = dkeys[(size_t)i]; t_improved[(size_t)i] = t; i_improved[(size_t)i] = iters_done; }
            keys[(size_t)i] = std::min(dkeys[(size_t)i], inc_key[(size_t)i]);
            if (keys[(size_t)i] < prev[(size_t)i]) { prev[(size_t)i] = keys[(size_t)i]; t_best[(size_t)i] = t; t_last_improve = t; }
        }
        all_done = check_done();
        const double t_search = now_s();
        if ((rc = service_bound(false))) return rc;
        if (trace && now_s() - t_search > 2e-3) std::fprintf(stderr, "[kao-solve]   service_bound took %.3f ms\n", (now_s() - t_search) * 1e3);
        if ((rc = service_lp())) return rc;
        const double t_bound = now_s();
        const int cx0 = cx_calls;
        if (cx_on && !all_done && !has_target && (rc = cycles(t))) return rc;
        if (gens_on && !all_done && (rc = maybe_new_generation())) return rc;
        if (trace) {
            const double t_end = now_s();
            int64_t obj0 = feasible(0) ? objective(0) : -1;
            std::fprintf(stderr, "[kao-solve] launch %d t %.4f search+sync %.3f ms, bound service %.3f ms (last K-bound launch %.3f ms / %d it, next %d it), cx %d calls %.3f ms | topic0 obj %lld ub %lld\n",
                         launches, t_end - t0, (t_search - t_prev) * 1e3, (t_bound - t_search) * 1e3, s->bound_ms_last, s->bound_iters_last, dual_now,
                         cx_calls - cx0, (t_end - t_bound) * 1e3, (long long)obj0, (long long)s->ub[0]);
            if (gens_on) std::fprintf(stderr, "[kao-solve]   generation %d, its best %lld\n", generations, gfeasible(0) ? (long long)gobjective(0) : -1ll);
            t_prev = t_end;
        }
        return KAO_OK;
    }
    // K-bound runs beside the search on its own stream; when a launch has finished its certificates are merged and, while
    // some feasible incumbent is still below its bound, the next launch starts (aimed at the new incumbents).  Launch length
    // adapts so that one launch takes about 10 ms.  Called after every K-search launch and between the rounds of KAO-CX.
    int service_bound(bool start_now = true) {
        if (has_target || dual_iters <= 0) return KAO_OK;
        int rc;
        if (!det) {   // wall-clock schedule: a K-bound launch is merged whenever it happens to have finished
            const int busy = kao_session_bound_busy(s);
            if (busy < 0) return busy;
            if (busy) return KAO_OK;
        }
        if (s->bound_inflight) {
            if ((rc = kao_session_bounds(s, nullptr, nullptr, nullptr))) return rc;   // deterministic schedule: waits for the launch
            share_bounds();
            for (int i = 0; i < n; ++i) {
                if (!bound_ran[(size_t)i]) continue;
                ++bound_merges[(size_t)i];
                if (s->ub[(size_t)i] < ub_seen[(size_t)i]) { ub_seen[(size_t)i] = s->ub[(size_t)i]; bound_quiet[(size_t)i] = 0; }
                else ++bound_quiet[(size_t)i];
            }
            // the finished launch's multipliers (rounded to quarters) become the prices of the next K-search launches
            if (use_prices && (rc = kao_session_adopt_prices(s))) return rc;
            if (!det && s->bound_ms_last > 0) {
                const double scale = 10.0 / s->bound_ms_last;
                dual_now = (int)std::min(4096.0, std::max(32.0, s->bound_iters_last * std::min(4.0, std::max(0.25, scale))));
            }
            all_done = check_done();
        }
        bool any = false;
        for (int i = 0; i < n && !all_done; ++i) {
            const bool want = feasible(i) && objective(i) < s->ub[(size_t)i] && s->dual_ok[(size_t)i] && !s->topic_infeasible[(size_t)i] &&
                              !(s->dual_flags[(size_t)i] & 6) && !lp_certified[(size_t)i] &&   // (a topic KAO-LP has certified: K-bound cannot get below the LP value)
                              !(lp_state[(size_t)i] == 1 && lp_all[(size_t)i]);                // (a huge topic while its LP runs: the search is paused, prices have no reader)
            bool rest = false;
            if (want && det && bound_quiet[(size_t)i] >= bound_quiet_max &&
                (int64_t)topics[i].n_partitions * topics[i].rf > bound_rest_slots)
                rest = (++bound_turn[(size_t)i] % bound_duty) != 0;
            dual_target[(size_t)i] = want && !rest ? objective(i) : -1;
            bound_ran[(size_t)i] = want && !rest;
            any |= want && !rest;
        }
        bound_pending = false;
        if (any) {
            if (det && !start_now) bound_pending = true;   // goes out behind the next K-search launch (launch())
            else if ((rc = kao_session_bound_step(s, dual_target.data(), dual_now))) return rc;
        }
        return KAO_OK;
    }
    // between the rounds of KAO-CX K-bound is serviced.  (Keeping K-search running as well -- launches enqueued from here
    // whenever its stream had drained -- was measured and dropped: 300 x 2000, 8 seeds, 3 s: mean 14823.5 with, 14824.4 without.)
    static int poll_bound(void *self) { return static_cast<SolveRun *>(self)->service_bound(); }
    // KAO-CX for feasible, unproven topics whose search has stalled (no improvement for 50 ms) or that have not been looked at
    // for 250 ms: the incumbent goes through kao_cycle.hip to a fixpoint of the cyclic-exchange neighbourhood and, when that
    // improved it, comes back as the topic's incumbent (elite launches re-seed the restarts from it)
    int cycles(double t) {
        for (int i = 0; i < n; ++i) {
            if (s->topic_infeasible[(size_t)i] || !gfeasible(i) || (feasible(i) && objective(i) >= s->ub[(size_t)i])) continue;
            if (!cycle_supported(&topics[i])) continue;
            if (lp_state[(size_t)i] == 1 && lp_all[(size_t)i]) continue;   // a huge topic's LP has the GPU to itself (beside it a round takes 20 ms instead of 8)
            if (lp_round_on && lp_possible(i) && !lp_try[(size_t)i] && (int64_t)topics[i].n_partitions * topics[i].rf >= lp_mid_slots &&
                !lp_waits_for_cx(i)) continue;   // (round 6) its first LP is waiting or running: the rounded iterate comes first
            const bool elite_fresh = (dkeys[(size_t)i] >> 20) != (cx_seen[(size_t)i] >> 20);   // not the incumbent of the last fixpoint
            const bool more = det && cx_starts > 0;
            if (!elite_fresh && !more) continue;
            if (det) {   // counts, not the clock: iterations since the last improvement / since the last call
                const bool stalled = iters_done - i_improved[(size_t)i] >= cx_stall_iters, due = iters_done - i_cx[(size_t)i] >= cx_due_iters;
                if (!cx_eager && (!(stalled || due) || iters_done - i_cx[(size_t)i] < cx_stall_iters)) continue;
            } else {
                const bool stalled = t - t_improved[(size_t)i] >= 0.05, due = t - t_cx[(size_t)i] >= 2.0 * cx_slice;
                if (!cx_eager && (t < 0.05 || !(stalled || due) || t - t_cx[(size_t)i] < 0.05)) continue;
            }
            const size_t slots = (size_t)topics[i].n_partitions * topics[i].rf;
            cx_buf.resize(slots);
            int rc;
            if (!cx_ctx[(size_t)i] && !(cx_ctx[(size_t)i] = cycle_open(&topics[i], &rc))) return rc;
            if (elite_fresh) {
                if ((rc = session_topic_best(s, i, cx_buf.data()))) return rc;
                if (more) cx_started[(size_t)i].push_back(start_hash(cx_buf.data(), slots));
                if ((rc = cycle_start(i, gobjective(i), det ? cx_rounds : 0, true))) return rc;
            }
            if (more && !(feasible(i) && objective(i) >= s->ub[(size_t)i]) && now_s() < deadline && (rc = further_starts(i))) return rc;
            // a context holds ~90 B per broker pair on the device and as much on the host: keep a handful, not one per topic
            int open = 0;
            for (CycleCtx *c : cx_ctx) open += c != nullptr;
            if (open > 8) { cycle_close(cx_ctx[(size_t)i]); cx_ctx[(size_t)i] = nullptr; }
        }
        all_done = check_done();
        return KAO_OK;
    }
    static uint64_t start_hash(const uint16_t *a, size_t n) {   // FNV-1a over the slots
        uint64_t h = 1469598103934665603ull;
        for (size_t k = 0; k < n; ++k) { h ^= a[k]; h *= 1099511628211ull; }
        return h;
    }
    // KAO-CX from the assignment in cx_buf (objective obj0) for at most `rounds` rounds; a result better than the generation's
    // incumbent becomes the topic's incumbent and elite
    int cycle_start(int i, int64_t obj0, int rounds, bool is_elite, int64_t *reached = nullptr) {
        int64_t obj = obj0;
        int32_t st[8];
        // the clock only ends a deterministic call at the solve's own deadline (the stop condition)
        const double slice_end = det ? deadline : std::min(deadline, now_s() + cx_slice);
        int rc = cycle_run(cx_ctx[(size_t)i], cx_buf.data(), rounds, slice_end, &obj, st, &SolveRun::poll_bound, this, is_elite);
        ++cx_calls;
        if (rc) return rc;
        if (reached) *reached = obj;
        if (trace) std::fprintf(stderr, "[kao-solve]   KAO-CX topic %d %s start %lld -> %lld in %d rounds (%d improving), incumbent %lld, launch %d\n", i, is_elite ? "elite" : "further",
                                (long long)obj0, (long long)obj, st[0], st[1], (long long)gobjective(i), launches);
        const bool fixpoint = st[0] > st[1];   // the last round found nothing
        const double t2 = now_s() - t0;
        t_cx[(size_t)i] = t2;
        i_cx[(size_t)i] = iters_done;
        if (obj > gobjective(i)) {
            uint64_t key = 0;
            if ((rc = session_adopt_external(s, i, cx_buf.data(), obj, &key))) return rc;
            dkeys[(size_t)i] = gprev[(size_t)i] = key;
            t_improved[(size_t)i] = t2;
            i_improved[(size_t)i] = iters_done;
            if (key < keys[(size_t)i]) { keys[(size_t)i] = prev[(size_t)i] = key; t_best[(size_t)i] = t_last_improve = t2; }
            ++cx_gains;
            if (fixpoint) cx_seen[(size_t)i] = key;
        } else if (fixpoint && is_elite) cx_seen[(size_t)i] = dkeys[(size_t)i];   // the incumbent itself is a fixpoint
        return KAO_OK;
    }
    // Further starting points (deterministic schedule): independent descents end a unit or two apart -- which basin KAO-CX
    // lands in is decided by where it starts (drifted 300 x 2000, scalar replay + oracle: 16 single restarts of 25,600
    // iterations -> fixpoints 14810..14826, three of them the optimum 14826) -- so besides the elite the best snapshots of the
    // best other restarts (by their own best objective, ties to the lower index; an assignment is started from once per
    // generation) are run to a fixpoint too.  Only a result that beats the incumbent is adopted.  The first call of a
    // generation meets the most diverse population (nothing has been re-seeded from a KAO-CX result yet) and gets
    // `cx_starts_first` starts, later calls `cx_starts`; where the descents end far below the incumbent (slack bands: drifted
    // 400 x 3000, fixpoints 25-60 units short) they only take time from the search, so a call whose first four starts all end
    // more than a unit below the incumbent stops there and the next call of the topic gets a quarter of the budget.
    int further_starts(int i) {
        int rc = session_restart_objs(s, i, start_objs);
        if (rc) return rc;
        const int nr = (int)start_objs.size();
        start_order.resize((size_t)nr);
        for (int r = 0; r < nr; ++r) start_order[(size_t)r] = r;
        std::stable_sort(start_order.begin(), start_order.end(), [&](int a, int b) { return start_objs[(size_t)a] > start_objs[(size_t)b]; });
        const size_t slots = (size_t)topics[i].n_partitions * topics[i].rf;
        const int budget = start_budget[(size_t)i];
        const int64_t inc0 = gobjective(i);
        int done = 0, near = 0, gains = 0;
        for (int q = 0; q < nr && done < budget; ++q) {
            const int r = start_order[(size_t)q];
            if (start_objs[(size_t)r] < 0) break;
            if (feasible(i) && objective(i) >= s->ub[(size_t)i]) break;
            if (now_s() >= deadline) break;
            if ((rc = session_restart_best(s, i, r, cx_buf.data()))) return rc;
            const uint64_t h = start_hash(cx_buf.data(), slots);
            std::vector<uint64_t> &seen = cx_started[(size_t)i];
            if (std::find(seen.begin(), seen.end(), h) != seen.end()) continue;
            seen.push_back(h);
            ++done; ++cx_more;
            int64_t reached = -1;
            if ((rc = cycle_start(i, start_objs[(size_t)r], cx_start_rounds, false, &reached))) return rc;
            near += reached >= inc0 - 1;
            gains += reached > inc0;
            if (done == 4 && near == 0) break;
        }
        if (done > 0) {
            // a batch pays when one of its descents beat the incumbent it met (restarts re-seeded from the elite end NEAR it by
            // construction); one that did not halves the next call's budget
            start_near[(size_t)i] += gains;
            start_budget[(size_t)i] = gains > 0 ? cx_starts : std::max(1, std::min(budget, cx_starts) / (near > 0 ? 2 : 4));
        }
        return KAO_OK;
    }
    // every open topic's population has converged (its best is a fixpoint of KAO-CX and nothing has improved since): bank the
    // incumbents and start the next generation
    int maybe_new_generation() {
        bool any_open = false;
        for (int i = 0; i < n; ++i) {
            if (topic_done(i)) continue;
            any_open = true;
            const int64_t quiet = iters_done - std::max(i_improved[(size_t)i], gen_start);
            const bool cx_ok = cycle_supported(&topics[i]) && gfeasible(i);
            if (cx_ok ? !((dkeys[(size_t)i] >> 20) == (cx_seen[(size_t)i] >> 20) && quiet >= gen_stall_iters) : quiet < cx_due_iters + gen_stall_iters) return KAO_OK;
        }
        if (!any_open) return KAO_OK;
        int rc;
        for (int i = 0; i < n; ++i) {
            if (dkeys[(size_t)i] >= inc_key[(size_t)i] || !gfeasible(i)) continue;
            inc_assign[(size_t)i].resize((size_t)topics[i].n_partitions * topics[i].rf);
            if ((rc = session_topic_best(s, i, inc_assign[(size_t)i].data()))) return rc;
            inc_key[(size_t)i] = dkeys[(size_t)i];
        }
        if ((rc = kao_session_new_generation(s))) return rc;
        ++generations;
        gen_start = iters_done;
        for (int i = 0; i < n; ++i) { dkeys[(size_t)i] = gprev[(size_t)i] = ~0ull; i_improved[(size_t)i] = i_cx[(size_t)i] = iters_done; cx_seen[(size_t)i] = ~0ull; cx_started[(size_t)i].clear();
            // a topic none of whose further starts came near the incumbent in the generation that ends gets a small first batch
            start_budget[(size_t)i] = start_near[(size_t)i] > 0 || cx_starts_first <= 4 ? cx_starts_first : 4; start_near[(size_t)i] = 0; }
        return KAO_OK;
    }
    int finish(kao_result *results, bool hit_time) {
        int rc = KAO_OK;
        if (s->bound_inflight && (rc = kao_session_bounds(s, nullptr, nullptr, nullptr))) return rc;  // last K-bound launch
        if ((rc = service_lp(true))) return rc;                                                        // an LP whose stop flag is up by now still counts
        share_bounds();
        std::vector<kao_result> rs((size_t)n);
        std::vector<std::vector<uint16_t>> bufs((size_t)n);
        for (int i = 0; i < n; ++i) {
            rs[(size_t)i] = kao_result{};
            bufs[(size_t)i].assign((size_t)xt[(size_t)i].n_partitions * std::max(xt[(size_t)i].rf, 1), (uint16_t)KAO_NONE);
            rs[(size_t)i].assignment = bufs[(size_t)i].data();
        }
        if ((rc = kao_session_best(s, rs.data()))) return rc;
        for (int i = 0; i < n; ++i) {   // an earlier generation's incumbent that the current one has not beaten is the answer
            const bool cur_ok = rs[(size_t)i].status != KAO_STATUS_NO_FEASIBLE && rs[(size_t)i].status != KAO_STATUS_INFEASIBLE_PROVEN;
            if (inc_key[(size_t)i] == ~0ull || (inc_key[(size_t)i] >> 44) != 0) continue;
            const int64_t inc_obj = (int64_t)kObjCap - (int64_t)((inc_key[(size_t)i] >> 20) & 0xFFFFFF);
            if (cur_ok && rs[(size_t)i].objective >= inc_obj) continue;
            kao_result &r = rs[(size_t)i];
            r.objective = inc_obj; r.best_restart = -1;
            std::memset(r.violations, 0, sizeof r.violations);
            bufs[(size_t)i] = inc_assign[(size_t)i];
            r.assignment = bufs[(size_t)i].data();
            r.status = r.objective >= r.upper_bound ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
        }
        auto better = [](const kao_result &a, const kao_result &b) {   // feasible first, then objective
            const bool fa = a.status != KAO_STATUS_NO_FEASIBLE && a.status != KAO_STATUS_INFEASIBLE_PROVEN;
            const bool fb = b.status != KAO_STATUS_NO_FEASIBLE && b.status != KAO_STATUS_INFEASIBLE_PROVEN;
            return fa != fb ? fa : a.objective > b.objective;
        };
        for (int i = 0; i < n;) {
            int best = i, j = i + 1;
            for (; j < n && origin[(size_t)j] == origin[(size_t)i]; ++j) if (better(rs[(size_t)j], rs[(size_t)best])) best = j;
            kao_result &out = results[origin[(size_t)i]];
            uint16_t *dst = out.assignment;
            out = rs[(size_t)best];
            out.assignment = dst;
            if (dst) std::memcpy(dst, bufs[(size_t)best].data(), bufs[(size_t)best].size() * 2);
            out.seconds_to_best = t_best[(size_t)best];
            if (hit_time && out.status == KAO_STATUS_FEASIBLE_BOUND_GAP) out.status = KAO_STATUS_TIME_LIMIT;
            i = j;
        }
        return rc;
    }
};

// kao_solve's defaults on top of the caller's options
kao_opts solve_defaults(const kao_topic *topics, int32_t n_topics, const kao_opts *opts) {
    kao_opts so{};
    if (opts) so = *opts;
    if (so.iters_per_launch <= 0) {
        // latency first (the host checks the bound after every launch): 128 iterations; large topics pay O(P) per launch
        // for loading, recounting and storing a restart (drifted 500 x 5000 topic: 40 % more iterations per second with
        // 512 per launch), so they get longer launches
        int64_t slots = 0;
        for (int i = 0; topics && i < n_topics; ++i) slots = std::max<int64_t>(slots, (int64_t)topics[i].n_partitions * std::max(topics[i].rf, 1));
        so.iters_per_launch = slots <= 4096 ? 128 : (slots <= 8192 ? 256 : 512);
    }
    if (so.elite_period == 0 && topics && n_topics > 0) {  // about one penalty period of the largest topic between elite launches
        int lg = 8;
        for (int i = 0; i < n_topics; ++i)
            lg = std::max(lg, so.period_log2 > 0 ? so.period_log2 : auto_period_log2(topics[i].n_partitions, std::max(topics[i].rf, 1)));
        so.elite_period = std::max(1, (1 << std::min(lg, 20)) / so.iters_per_launch);
    }
    return so;
}

}  // namespace

namespace kao {
int api_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
int api_require_init() { return require_init(); }
double api_now_s() { return now_s(); }
}  // namespace kao

extern "C" {

int kao_solve(const kao_topic *topics, int32_t n_topics, const kao_opts *opts, kao_result *results) {
    const double t0 = now_s();
    if (!results) return fail(KAO_ERR_INVALID, "null results");
    if (opts && (opts->team < 0 || opts->team > kTeamMax || opts->schedule < 0 || opts->schedule > 1)) return fail(KAO_ERR_INVALID, "kao_opts: team must be 0..8, schedule 0 or 1");
    const kao_opts so = solve_defaults(topics, n_topics, opts);
    SolveRun run;
    int rc = run.begin(topics, n_topics, so, opts ? opts->target_objective : nullptr, t0, true, true);
    if (rc) return rc;
    g_timing[0] = now_s() - t0;
    const kao_opts &o = run.s->opts;
    bool hit_time = false;
    for (;;) {
        if ((rc = run.launch()) || (rc = run.after_launch())) return rc;
        if (o.stop_at_bound && run.all_done) break;
        if (o.max_launches > 0 && run.launches >= o.max_launches) break;
        if (now_s() - t0 >= o.time_limit_s) { hit_time = true; break; }
    }
    g_timing[1] = run.t_last_improve;
    rc = run.finish(results, hit_time);
    g_timing[2] = now_s() - t0;
    g_timing[5] = (double)run.s->delta_total;
    g_timing[6] = (double)run.s->bound_launches;
    g_timing[7] = 0;   // elite exchanges between GPUs: none on one device
    g_timing[8] = 0;   // K-bound iterations, summed over the topics
    for (int32_t v : run.s->dual_iters) g_timing[8] += (double)v;
    g_timing[9] = run.cx_calls; g_timing[10] = run.cx_gains; g_timing[11] = (double)run.iters_done; g_timing[12] = run.generations;
    g_timing[13] = run.cx_more;
    g_timing[14] = run.lp_solves; g_timing[15] = run.lp_iters;
    g_lp[0] = run.lp_solves; g_lp[1] = run.lp_iters; g_lp[2] = run.lp_rounded; g_lp[3] = run.lp_round_adopted; g_lp[4] = run.lp_round_fractional;
    for (double &q : g_profile) q = 0;
    if (o.profile) {
        kao_stats st{};
        if (kao_session_stats(run.s, &st) == KAO_OK) {
            g_profile[0] = st.ms_search; g_profile[1] = st.ms_eval; g_profile[2] = (double)st.launches; g_profile[3] = st.n_restarts_total;
            g_profile[4] = (double)st.search_bytes_algo; g_profile[5] = (double)st.delta_candidates; g_profile[6] = st.lds_bytes_search; g_profile[7] = st.blocks_search;
        }
    }
    kao_session_destroy(run.s);
    run.s = nullptr;
    g_timing[3] = now_s() - t0;
    g_timing[4] = run.launches;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// kao_solve_multi: one process, several GPUs
// ------------------------------------------------------------------------------------------------
namespace {
// librccl.so is half a gigabyte of code objects; linking it would make every process that loads libkao.so (the CLI, a JVM)
// pay for registering them.  It is opened on the first multi-GPU exchange instead.
struct Rccl {
    void *h = nullptr;
    std::string why = "not found";   // text of the last dlopen / dlsym failure
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    bool load() {
        if (h) return true;
        // RCCL must sit on the SAME HIP / HSA runtime instance this library runs on (a process may hold two: PyTorch wheels
        // bundle their own next to /opt/rocm's): look for librccl next to the libamdhip64 that serves our HIP calls first
        std::vector<std::string> names;
        Dl_info info;
        if (dladdr(reinterpret_cast<void *>(&hipGetDeviceCount), &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) { dir.resize(slash); names.push_back(dir + "/librccl.so.1"); names.push_back(dir + "/librccl.so"); }
        }
        names.push_back("librccl.so.1"); names.push_back("librccl.so"); names.push_back("/opt/rocm/lib/librccl.so.1");
        for (const std::string &name : names) {
            h = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (h) break;
            if (const char *e = dlerror()) why = e;   // dlerror() clears the message: read it once, here
        }
        if (!h) return false;
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(h, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(h, "ncclCommDestroy"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(h, "ncclGetErrorString"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(h, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(h, "ncclGroupEnd"));
        AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(h, "ncclAllReduce"));
        Broadcast = reinterpret_cast<decltype(Broadcast)>(dlsym(h, "ncclBroadcast"));
        if (CommInitAll && CommDestroy && GetErrorString && GroupStart && GroupEnd && AllReduce && Broadcast) return true;
        if (const char *e = dlerror()) why = e; else why = "missing symbol";
        dlclose(h); h = nullptr;
        return false;
    }
} g_rccl;

// ---- loop-back collectives (test hook KAO_RCCL_LOOPBACK=1) ----------------------------------------------------------------
// The same function table filled with an in-process implementation: "ranks" are entries of the device list -- which may name
// one device several times -- and the two collectives kao_solve_multi uses move the data with plain copies when the group
// closes.  It exists so that the REAL control flow of the elite exchange (grouped ncclAllReduce(ncclUint64, ncclMin) on the
// resident key buffers, then one grouped ncclBroadcast per topic from the winner's rank) runs with several communicators on a
// box that has one GPU (the grouped sequence had never executed with more than one rank).  Never used unless the
// environment asks for it; results are those RCCL would deliver.
struct LoopComm { int rank, nranks, device; };
struct LoopOp { int kind; const void *send; void *recv; size_t count; int dtype, root; LoopComm *comm; hipStream_t st; int op; };
thread_local std::vector<LoopOp> t_loop_ops;
thread_local int t_loop_depth = 0;
uint64_t g_loop_allreduces = 0, g_loop_broadcasts = 0;   // collectives completed (test hook kao_rccl_loopback_counts)
size_t loop_elem(int dtype) { return dtype == ncclUint64 || dtype == ncclInt64 || dtype == ncclDouble ? 8 : (dtype == ncclUint8 || dtype == ncclInt8 ? 1 : 4); }
ncclResult_t loop_run() {
    std::vector<LoopOp> ops;
    ops.swap(t_loop_ops);
    if (ops.empty()) return ncclSuccess;
    const int n = ops[0].comm->nranks;
    if ((int)ops.size() != n) return ncclInvalidUsage;            // every rank of the communicator must take part
    std::vector<const LoopOp *> by_rank((size_t)n, nullptr);
    for (const LoopOp &o : ops) {
        if (o.kind != ops[0].kind || o.count != ops[0].count || o.dtype != ops[0].dtype || o.root != ops[0].root || o.op != ops[0].op || o.comm->nranks != n) return ncclInvalidUsage;
        if (o.comm->rank < 0 || o.comm->rank >= n || by_rank[(size_t)o.comm->rank]) return ncclInvalidUsage;
        by_rank[(size_t)o.comm->rank] = &o;
    }
    const size_t bytes = ops[0].count * loop_elem(ops[0].dtype);
    for (const LoopOp &o : ops)   // a collective is ordered behind the work already enqueued on each rank's stream
        if (hipSetDevice(o.comm->device) != hipSuccess || hipStreamSynchronize(o.st) != hipSuccess) return ncclUnhandledCudaError;
    if (ops[0].kind == 0 && ops[0].dtype == ncclDouble) {   // f64 sum / min (KAO-LP's shards): added in RANK order, every rank gets the same bits
        std::vector<double> acc(ops[0].count), tmp(ops[0].count);
        for (int r = 0; r < n; ++r) {
            const LoopOp &o = *by_rank[(size_t)r];
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(r ? tmp.data() : acc.data(), o.send, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
            if (r) for (size_t i = 0; i < acc.size(); ++i) acc[i] = ops[0].op == (int)ncclMin ? std::min(acc[i], tmp[i]) : acc[i] + tmp[i];
        }
        for (const LoopOp &o : ops)
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(o.recv, acc.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
        ++g_loop_allreduces;
    } else if (ops[0].kind == 0) {   // all-reduce: uint64 / min (the elite exchange)
        if (ops[0].dtype != ncclUint64) return ncclInvalidArgument;
        std::vector<uint64_t> acc(ops[0].count, ~0ull), tmp(ops[0].count);
        for (const LoopOp &o : ops) {
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(tmp.data(), o.send, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
            for (size_t i = 0; i < acc.size(); ++i) acc[i] = std::min(acc[i], tmp[i]);
        }
        for (const LoopOp &o : ops)
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(o.recv, acc.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
        ++g_loop_allreduces;
    } else {                  // broadcast from rank `root`
        if (ops[0].root < 0 || ops[0].root >= n) return ncclInvalidArgument;
        std::vector<unsigned char> buf(bytes);
        const LoopOp &r = *by_rank[(size_t)ops[0].root];
        if (hipSetDevice(r.comm->device) != hipSuccess || hipMemcpy(buf.data(), r.send, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
        for (const LoopOp &o : ops)
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(o.recv, buf.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
        ++g_loop_broadcasts;
    }
    return ncclSuccess;
}
ncclResult_t loop_CommInitAll(ncclComm_t *comms, int ndev, const int *devlist) {
    for (int i = 0; i < ndev; ++i) comms[i] = reinterpret_cast<ncclComm_t>(new LoopComm{i, ndev, devlist ? devlist[i] : i});
    return ncclSuccess;
}
ncclResult_t loop_CommDestroy(ncclComm_t c) { delete reinterpret_cast<LoopComm *>(c); return ncclSuccess; }
const char *loop_GetErrorString(ncclResult_t r) { return r == ncclSuccess ? "no error" : (r == ncclInvalidUsage ? "loop-back: invalid usage (a rank is missing from the group)" : "loop-back: error"); }
ncclResult_t loop_GroupStart() { ++t_loop_depth; return ncclSuccess; }
ncclResult_t loop_GroupEnd() { if (t_loop_depth <= 0) return ncclInvalidUsage; return --t_loop_depth == 0 ? loop_run() : ncclSuccess; }
ncclResult_t loop_AllReduce(const void *send, void *recv, size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm_t c, hipStream_t st) {
    if (!((dt == ncclUint64 && op == ncclMin) || (dt == ncclDouble && (op == ncclMin || op == ncclSum)))) return ncclInvalidArgument;
    t_loop_ops.push_back(LoopOp{0, send, recv, count, (int)dt, 0, reinterpret_cast<LoopComm *>(c), st, (int)op});
    return t_loop_depth == 0 ? loop_run() : ncclSuccess;
}
ncclResult_t loop_Broadcast(const void *send, void *recv, size_t count, ncclDataType_t dt, int root, ncclComm_t c, hipStream_t st) {
    t_loop_ops.push_back(LoopOp{1, send, recv, count, (int)dt, root, reinterpret_cast<LoopComm *>(c), st, 0});
    return t_loop_depth == 0 ? loop_run() : ncclSuccess;
}
struct LoopTable : Rccl {
    LoopTable() {
        CommInitAll = &loop_CommInitAll; CommDestroy = &loop_CommDestroy; GetErrorString = &loop_GetErrorString;
        GroupStart = &loop_GroupStart; GroupEnd = &loop_GroupEnd; AllReduce = &loop_AllReduce; Broadcast = &loop_Broadcast;
    }
} g_loop;
bool loopback_wanted() { return env_int("KAO_RCCL_LOOPBACK", 0) != 0; }

struct CommSet { std::vector<int> devices; const Rccl *api; std::vector<ncclComm_t> comms; };
std::vector<CommSet> g_comms;   // communicators per (device list, function table) (creation costs ~100 ms with RCCL; kept until kao_shutdown)
std::mutex g_comm_mu;
int comms_for(const std::vector<int> &devices, std::vector<ncclComm_t> &out, const Rccl **api_out) {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    const bool loop = loopback_wanted();
    const Rccl *api = loop ? &g_loop : &g_rccl;
    *api_out = api;
    for (const CommSet &c : g_comms) if (c.devices == devices && c.api == api) { out = c.comms; return KAO_OK; }
    if (!loop && !g_rccl.load()) return fail(KAO_ERR_HIP, std::string("librccl.so not available: ") + g_rccl.why);
    for (int d : devices) {  // RCCL expects every device's primary context to exist already
        if (hipSetDevice(d) != hipSuccess || hipFree(nullptr) != hipSuccess) return fail(KAO_ERR_HIP, "cannot initialise device " + std::to_string(d));
        void *probe = nullptr;
        if (hipMalloc(&probe, 256) == hipSuccess) (void)hipFree(probe);
    }
    if (cur_device() >= 0) (void)hipSetDevice(cur_device());
    CommSet c; c.devices = devices; c.api = api; c.comms.resize(devices.size());
    const ncclResult_t r = api->CommInitAll(c.comms.data(), (int)devices.size(), devices.data());
    if (r != ncclSuccess) return fail(KAO_ERR_HIP, std::string("ncclCommInitAll: ") + api->GetErrorString(r));
    g_comms.push_back(c);
    out = c.comms;
    return KAO_OK;
}
}  // namespace

void kao_multi_shutdown_comms(void) {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    for (CommSet &c : g_comms) for (ncclComm_t cm : c.comms) (void)c.api->CommDestroy(cm);
    g_comms.clear();
}

// Diagnostic: the collectives kao_solve_multi uses, on small resident buffers of the listed (distinct) devices -- rank r holds
// keys {100 - r, 7 + r, ~0, r}; after ncclAllReduce(ncclUint64, ncclMin) every rank must hold {101 - n, 7, ~0, 0}, and after
// ncclBroadcast from the last rank every rank holds that rank's 64-byte pattern.  0 = ok.
int kao_rccl_selftest(const int32_t *devices, int32_t n_dev) {
    if (!devices || n_dev < 1 || n_dev > kMaxDevices) return fail(KAO_ERR_INVALID, "bad device list");
    std::vector<int> devs(devices, devices + n_dev);
    std::vector<ncclComm_t> comms;
    const Rccl *api = nullptr;
    int rc = comms_for(devs, comms, &api);
    if (rc) return rc;
    const Rccl &cc = *api;   // RCCL, or the loop-back table (KAO_RCCL_LOOPBACK=1: the list may then repeat a device)
    std::vector<unsigned long long *> keys((size_t)n_dev, nullptr), out((size_t)n_dev, nullptr);
    std::vector<unsigned char *> pat((size_t)n_dev, nullptr);
    std::vector<hipStream_t> st((size_t)n_dev, nullptr);
    bool ok = true;
    for (int d = 0; d < n_dev && ok; ++d) {
        ok = hipSetDevice(devs[(size_t)d]) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&keys[(size_t)d]), 32) == hipSuccess &&
             hipMalloc(reinterpret_cast<void **>(&out[(size_t)d]), 32) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&pat[(size_t)d]), 64) == hipSuccess &&
             hipStreamCreateWithFlags(&st[(size_t)d], hipStreamNonBlocking) == hipSuccess;
        const unsigned long long h[4] = {100ull - (unsigned)d, 7ull + (unsigned)d, ~0ull, (unsigned long long)d};
        unsigned char p[64];
        for (int i = 0; i < 64; ++i) p[i] = (unsigned char)(d * 64 + i);
        ok = ok && hipMemcpy(keys[(size_t)d], h, 32, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(pat[(size_t)d], p, 64, hipMemcpyHostToDevice) == hipSuccess;
    }
    ncclResult_t nr = ok ? cc.GroupStart() : ncclSystemError;
    for (int d = 0; d < n_dev && nr == ncclSuccess; ++d) nr = cc.AllReduce(keys[(size_t)d], out[(size_t)d], 4, ncclUint64, ncclMin, comms[(size_t)d], st[(size_t)d]);
    if (nr == ncclSuccess) nr = cc.GroupEnd();
    if (nr == ncclSuccess) nr = cc.GroupStart();
    for (int d = 0; d < n_dev && nr == ncclSuccess; ++d) nr = cc.Broadcast(pat[(size_t)d], pat[(size_t)d], 64, ncclUint8, n_dev - 1, comms[(size_t)d], st[(size_t)d]);
    if (nr == ncclSuccess) nr = cc.GroupEnd();
    ok = ok && nr == ncclSuccess;
    for (int d = 0; d < n_dev && ok; ++d) {
        unsigned long long h[4]; unsigned char p[64];
        ok = hipSetDevice(devs[(size_t)d]) == hipSuccess && hipStreamSynchronize(st[(size_t)d]) == hipSuccess &&
             hipMemcpy(h, out[(size_t)d], 32, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(p, pat[(size_t)d], 64, hipMemcpyDeviceToHost) == hipSuccess;
        ok = ok && h[0] == 101ull - (unsigned)n_dev && h[1] == 7ull && h[2] == ~0ull && h[3] == 0ull;
        for (int i = 0; i < 64 && ok; ++i) ok = p[i] == (unsigned char)((n_dev - 1) * 64 + i);
    }
    for (int d = 0; d < n_dev; ++d) {
        (void)hipSetDevice(devs[(size_t)d]);
        (void)hipFree(keys[(size_t)d]); (void)hipFree(out[(size_t)d]); (void)hipFree(pat[(size_t)d]);
        if (st[(size_t)d]) (void)hipStreamDestroy(st[(size_t)d]);
    }
    if (cur_device() >= 0) (void)hipSetDevice(cur_device());
    if (!ok) return fail(KAO_ERR_HIP, nr != ncclSuccess ? std::string("RCCL: ") + cc.GetErrorString(nr) : std::string("RCCL self-test: wrong result"));
    return KAO_OK;
}

int kao_solve_multi(const kao_topic *topics, int32_t n_topics, const int32_t *devices, int32_t n_dev, const kao_opts *opts,
                    kao_result *results) {
    const double t0 = now_s();
    if (!topics || n_topics < 1 || !results) return fail(KAO_ERR_INVALID, "no topics / null results");
    if (!devices || n_dev < 1 || n_dev > kMaxDevices) return fail(KAO_ERR_INVALID, "bad device list");
    if (opts && (opts->team < 0 || opts->team > kTeamMax || opts->schedule < 0 || opts->schedule > 1)) return fail(KAO_ERR_INVALID, "kao_opts: team must be 0..8, schedule 0 or 1");
    int n_hw = 0;
    if (hipGetDeviceCount(&n_hw) != hipSuccess || n_hw <= 0) return fail(KAO_ERR_NO_DEVICE, "no HIP device");
    std::vector<int> devs(devices, devices + n_dev);
    bool distinct = true;
    for (int i = 0; i < n_dev; ++i) {
        if (devs[(size_t)i] < 0 || devs[(size_t)i] >= n_hw) return fail(KAO_ERR_INVALID, "device ordinal out of range");
        for (int j = 0; j < i; ++j) distinct &= devs[(size_t)j] != devs[(size_t)i];
    }
    if (!is_init()) { int rc0 = kao_init(devs[0]); if (rc0) return rc0; }
    if (n_dev == 1) {   // a list of one device: exactly kao_solve (generations, islands), on THAT device (callers used to
                        // fall back to the kao_init device and ignore the ordinal they had been given)
        const int saved = t_device;
        t_device = devs[0];
        const int rc1 = kao_solve(topics, n_topics, opts, results);
        t_device = saved;
        if (cur_device() >= 0) (void)hipSetDevice(cur_device());
        return rc1;
    }
    const kao_opts so = solve_defaults(topics, n_topics, opts);
    const bool replicated = n_topics < n_dev;   // fewer topics than GPUs: every GPU searches every topic, elites are exchanged
    bool race = false;
    for (int i = 0; replicated && i < n_topics; ++i) race |= (int64_t)topics[i].n_partitions * topics[i].rf >= 32768;
    // KAO_MULTI_LP=shard (opt-in, round 6): instead of racing whole solves, ONE LP of such a topic runs sharded by partition range over all
    // devices (driven by device 0's solve loop through lp_open_fan; the other devices' loops launch no K-search while it has the GPUs).
    // Exercised on logical shards only (tests/test_gpu_parity.py); the race stays the default until a multi-GPU node has timed both.
    bool shard_lp = false, lp_pause = false;
    { const char *e = env_str("KAO_MULTI_LP"); shard_lp = race && e && e[0] == 's' && (distinct || loopback_wanted()); }
    // ---- shards: LPT by brokers x partitions (independent sub-problems, README.md:146-184) ----
    std::vector<std::vector<int>> shard((size_t)n_dev);
    if (replicated) for (auto &sh : shard) for (int i = 0; i < n_topics; ++i) sh.push_back(i);
    else {
        std::vector<int> order((size_t)n_topics);
        for (int i = 0; i < n_topics; ++i) order[(size_t)i] = i;
        auto size_of = [&](int i) { return (int64_t)topics[i].n_brokers * topics[i].n_partitions; };
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return size_of(a) > size_of(b); });
        std::vector<int64_t> load((size_t)n_dev, 0);
        for (int i : order) {
            int best = 0;
            for (int d = 1; d < n_dev; ++d) if (load[(size_t)d] < load[(size_t)best]) best = d;
            shard[(size_t)best].push_back(i);
            load[(size_t)best] += size_of(i);
        }
    }
    std::vector<ncclComm_t> comms;
    // logical shards on one device (tests) merge through plain copies -- or, with KAO_RCCL_LOOPBACK=1, through the same grouped
    // collective calls as distinct devices, served by the in-process loop-back table
    const bool use_rccl = replicated && (distinct || loopback_wanted());
    const Rccl *api = nullptr;
    if (use_rccl) { int rc0 = comms_for(devs, comms, &api); if (rc0) return rc0; }

    struct Dev { SolveRun run; std::vector<kao_topic> tp; std::vector<kao_result> res; std::vector<int64_t> tgt; };
    std::vector<Dev> D((size_t)n_dev);
    const int saved_t_device = t_device;
    auto cleanup = [&]() { t_device = saved_t_device; if (cur_device() >= 0) (void)hipSetDevice(cur_device()); };
    int rc = KAO_OK;
    for (int d = 0; d < n_dev && !rc; ++d) {
        Dev &x = D[(size_t)d];
        for (int i : shard[(size_t)d]) { x.tp.push_back(topics[i]); if (opts && opts->target_objective) x.tgt.push_back(opts->target_objective[i]); }
        if (x.tp.empty()) continue;
        kao_opts o = so;
        o.seed = so.seed + 0x9E3779B97F4A7C15ull * (uint64_t)d;            // replicated topics: a different seed per GPU
        // one certificate per topic is enough: device 0 runs K-bound.  Except in the LP's regime (round 6): a topic of lp_solo_slots replica
        // slots or more is solved by ONE perturbed interior-point solve whose iteration count is heavy-tailed (105 .. 200 at 100,000
        // partitions, depending on the perturbation's salt and on rounding noise) -- there every device runs the solve with its own salt and
        // the first proof ends the solve for all (certificates and incumbents are shared as before): a race, not a split of the work
        if (replicated && d > 0 && (!race || shard_lp)) o.dual_iters = -1;
        x.run.lp_salt0 = replicated ? d : 0;
        if (shard_lp) { if (d == 0) x.run.lp_fan_devs = devs; else x.run.ext_pause = &lp_pause; }
        t_device = devs[(size_t)d];
        if (hipSetDevice(t_device) != hipSuccess) { rc = fail(KAO_ERR_NO_DEVICE, "hipSetDevice"); break; }
        rc = x.run.begin(x.tp.data(), (int)x.tp.size(), o, x.tgt.empty() ? nullptr : x.tgt.data(), t0);
    }
    if (rc) { cleanup(); return rc; }
    g_timing[0] = now_s() - t0;
    const int exch = std::max(1, so.elite_period);
    bool hit_time = false;
    int rounds = 0;
    uint64_t exchanges = 0;
    std::vector<uint64_t> gmin((size_t)n_topics);
    std::vector<int> root((size_t)n_topics);
    for (;;) {
        if (shard_lp && D[0].run.s) lp_pause = D[0].run.search_paused();
        for (int d = 0; d < n_dev && !rc; ++d) if (D[(size_t)d].run.s) { t_device = devs[(size_t)d]; rc = D[(size_t)d].run.launch(); }
        for (int d = 0; d < n_dev && !rc; ++d) if (D[(size_t)d].run.s) { t_device = devs[(size_t)d]; rc = D[(size_t)d].run.after_launch(); }
        if (rc) break;
        ++rounds;
        if (replicated) {
            // certificates: any GPU's bound is valid for the topic
            for (int i = 0; i < n_topics; ++i) {
                int64_t ub = INT64_MAX;
                for (Dev &x : D) ub = std::min(ub, x.run.s->ub[(size_t)i]);
                for (Dev &x : D) x.run.s->ub[(size_t)i] = ub;
            }
            if (rounds % exch == 0 || so.stop_at_bound) {
                // ---- elite exchange: min-allreduce of the packed best keys on the resident buffers, winners broadcast ----
                bool differ = false;
                for (int i = 0; i < n_topics; ++i) {
                    gmin[(size_t)i] = ~0ull; root[(size_t)i] = 0;
                    for (int d = 0; d < n_dev; ++d) {
                        const uint64_t k = D[(size_t)d].run.keys[(size_t)i] | 0;  // host copy read by after_launch
                        if (k < gmin[(size_t)i]) { gmin[(size_t)i] = k; root[(size_t)i] = d; }
                    }
                    for (int d = 0; d < n_dev; ++d) differ |= (D[(size_t)d].run.keys[(size_t)i] >> 20) != (gmin[(size_t)i] >> 20);
                }
                if (differ && rounds % exch == 0) {
                    ++exchanges;
                    for (int d = 0; d < n_dev && !rc; ++d) {   // stage every GPU's current winners
                        kao_session *s = D[(size_t)d].run.s;
                        if (hipSetDevice(s->device) != hipSuccess) { rc = fail(KAO_ERR_HIP, "hipSetDevice"); break; }
                        launch_gather(s->d_topics, s->n_topics, s->d_keys, s->d_best, s->d_viol, s->d_win_assign, s->d_win_viol, s->stream);
                    }
                    if (!rc && use_rccl) {
                        ncclResult_t nr = api->GroupStart();
                        for (int d = 0; d < n_dev && nr == ncclSuccess; ++d) {
                            kao_session *s = D[(size_t)d].run.s;
                            nr = api->AllReduce(s->d_keys, s->d_keys_glob, (size_t)n_topics, ncclUint64, ncclMin, comms[(size_t)d], s->stream);
                        }
                        if (nr == ncclSuccess) nr = api->GroupEnd();
                        for (int i = 0; i < n_topics && nr == ncclSuccess; ++i) {
                            if ((gmin[(size_t)i] >> 44) != 0) continue;   // no feasible assignment anywhere yet
                            nr = api->GroupStart();
                            for (int d = 0; d < n_dev && nr == ncclSuccess; ++d) {
                                kao_session *s = D[(size_t)d].run.s;
                                const TopicDev &td = s->pts[(size_t)i].d;
                                uint16_t *buf = s->d_win_assign + td.win_off;
                                nr = api->Broadcast(buf, buf, (size_t)td.P * td.RF * 2, ncclUint8, root[(size_t)i], comms[(size_t)d], s->stream);
                            }
                            if (nr == ncclSuccess) nr = api->GroupEnd();
                        }
                        if (nr != ncclSuccess) rc = fail(KAO_ERR_HIP, std::string("RCCL elite exchange: ") + api->GetErrorString(nr));
                    } else if (!rc) {   // logical shards on one device: same data movement through plain copies
                        for (int d = 0; d < n_dev && !rc; ++d) {
                            kao_session *s = D[(size_t)d].run.s;
                            if (hipSetDevice(s->device) != hipSuccess) { rc = fail(KAO_ERR_HIP, "hipSetDevice"); break; }
                            for (int r2 = 0; r2 < n_dev; ++r2) (void)hipStreamSynchronize(D[(size_t)r2].run.s->stream);
                            if (hipMemcpyAsync(s->d_keys_glob, gmin.data(), (size_t)n_topics * 8, hipMemcpyHostToDevice, s->stream) != hipSuccess) rc = fail(KAO_ERR_HIP, "hipMemcpyAsync");
                            for (int i = 0; i < n_topics && !rc; ++i) {
                                if ((gmin[(size_t)i] >> 44) != 0 || root[(size_t)i] == d) continue;
                                kao_session *sr = D[(size_t)root[(size_t)i]].run.s;
                                const TopicDev &td = s->pts[(size_t)i].d;
                                if (hipMemcpyAsync(s->d_win_assign + td.win_off, sr->d_win_assign + td.win_off, (size_t)td.P * td.RF * 2,
                                                   hipMemcpyDeviceToDevice, s->stream) != hipSuccess) rc = fail(KAO_ERR_HIP, "hipMemcpyAsync");
                            }
                            if (!rc && hipStreamSynchronize(s->stream) != hipSuccess) rc = fail(KAO_ERR_HIP, "hipStreamSynchronize");  // gmin is reused
                        }
                    }
                    for (int d = 0; d < n_dev && !rc; ++d) {
                        kao_session *s = D[(size_t)d].run.s;
                        if (hipSetDevice(s->device) != hipSuccess) { rc = fail(KAO_ERR_HIP, "hipSetDevice"); break; }
                        launch_adopt_global(s->d_keys, s->d_keys_glob, n_topics, s->stream);
                        if (hipGetLastError() != hipSuccess) rc = fail(KAO_ERR_HIP, "k_adopt_global");
                    }
                    if (rc) break;
                }
                for (Dev &x : D)   // every run now judges "done" against the global incumbents
                    for (int i = 0; i < n_topics; ++i) if (gmin[(size_t)i] < x.run.keys[(size_t)i]) x.run.keys[(size_t)i] = gmin[(size_t)i];
                for (Dev &x : D) x.run.all_done = x.run.check_done();
            }
        }
        bool all = true;
        for (Dev &x : D) if (x.run.s) all &= x.run.all_done;
        if (replicated) { all = false; for (Dev &x : D) all |= x.run.all_done; }   // one GPU holding proven optima for every topic suffices
        if (so.stop_at_bound && all) break;
        if (so.max_launches > 0 && rounds >= so.max_launches) break;
        const double tl = so.time_limit_s > 0 ? so.time_limit_s : 10.0;
        if (now_s() - t0 >= tl) { hit_time = true; break; }
    }
    // ---- results ----
    double t_improve = 0, cand = 0, bl = 0;
    if (!rc) {
        if (replicated) {   // per topic: the GPU holding the best key answers
            std::vector<std::vector<kao_result>> rs((size_t)n_dev, std::vector<kao_result>((size_t)n_topics));
            std::vector<std::vector<std::vector<uint16_t>>> bufs((size_t)n_dev);
            for (int d = 0; d < n_dev && !rc; ++d) {
                bufs[(size_t)d].resize((size_t)n_topics);
                for (int i = 0; i < n_topics; ++i) {
                    bufs[(size_t)d][(size_t)i].assign((size_t)topics[i].n_partitions * topics[i].rf, (uint16_t)KAO_NONE);
                    rs[(size_t)d][(size_t)i] = kao_result{};
                    rs[(size_t)d][(size_t)i].assignment = bufs[(size_t)d][(size_t)i].data();
                }
                t_device = devs[(size_t)d];
                rc = D[(size_t)d].run.finish(rs[(size_t)d].data(), hit_time);
            }
            for (int i = 0; i < n_topics && !rc; ++i) {
                int best = 0;
                auto better = [&](const kao_result &a, const kao_result &b) {   // feasible first, then objective
                    const bool fa = a.status != KAO_STATUS_NO_FEASIBLE && a.status != KAO_STATUS_INFEASIBLE_PROVEN;
                    const bool fb = b.status != KAO_STATUS_NO_FEASIBLE && b.status != KAO_STATUS_INFEASIBLE_PROVEN;
                    return fa != fb ? fa : a.objective > b.objective;
                };
                for (int d = 1; d < n_dev; ++d) if (better(rs[(size_t)d][(size_t)i], rs[(size_t)best][(size_t)i])) best = d;
                uint16_t *dst = results[i].assignment;
                results[i] = rs[(size_t)best][(size_t)i];
                results[i].assignment = dst;
                if (dst) std::memcpy(dst, bufs[(size_t)best][(size_t)i].data(), bufs[(size_t)best][(size_t)i].size() * 2);
                int64_t ub = INT64_MAX;
                for (int d = 0; d < n_dev; ++d) ub = std::min(ub, rs[(size_t)d][(size_t)i].upper_bound);
                results[i].upper_bound = ub;
                if (results[i].status == KAO_STATUS_FEASIBLE_BOUND_GAP || results[i].status == KAO_STATUS_TIME_LIMIT || results[i].status == KAO_STATUS_OPTIMAL_PROVEN)
                    results[i].status = results[i].objective >= ub ? KAO_STATUS_OPTIMAL_PROVEN : (hit_time ? KAO_STATUS_TIME_LIMIT : KAO_STATUS_FEASIBLE_BOUND_GAP);
            }
        } else {
            for (int d = 0; d < n_dev && !rc; ++d) {
                Dev &x = D[(size_t)d];
                if (!x.run.s) continue;
                x.res.assign(x.tp.size(), kao_result{});
                for (size_t k = 0; k < x.tp.size(); ++k) x.res[k].assignment = results[shard[(size_t)d][k]].assignment;
                t_device = devs[(size_t)d];
                rc = x.run.finish(x.res.data(), hit_time);
                for (size_t k = 0; k < x.tp.size() && !rc; ++k) results[shard[(size_t)d][k]] = x.res[k];
            }
        }
    }
    g_timing[2] = now_s() - t0;
    for (int i = 8; i < 16; ++i) g_timing[i] = 0;   // counters of this call, summed over the devices (they kept the previous kao_solve's values)
    for (Dev &x : D) if (x.run.s) {
        t_improve = std::max(t_improve, x.run.t_last_improve); cand += (double)x.run.s->delta_total; bl += (double)x.run.s->bound_launches;
        for (int32_t v : x.run.s->dual_iters) g_timing[8] += (double)v;
        g_timing[9] += x.run.cx_calls; g_timing[10] += x.run.cx_gains; g_timing[11] += (double)x.run.iters_done;
        g_timing[12] += x.run.generations; g_timing[13] += x.run.cx_more;
        g_timing[14] += x.run.lp_solves; g_timing[15] += x.run.lp_iters;
    }
    for (double &q : g_lp) q = 0;     // KAO-LP over all devices (a replicated topic in the LP's regime is a race: every device runs its own solve)
    for (Dev &x : D) if (x.run.s) { g_lp[0] += x.run.lp_solves; g_lp[1] += x.run.lp_iters; g_lp[2] += x.run.lp_rounded; g_lp[3] += x.run.lp_round_adopted; g_lp[4] += x.run.lp_round_fractional; }
    for (int d = 0; d < n_dev; ++d) if (D[(size_t)d].run.s) { t_device = devs[(size_t)d]; kao_session_destroy(D[(size_t)d].run.s); D[(size_t)d].run.s = nullptr; }
    cleanup();
    g_timing[1] = t_improve; g_timing[3] = now_s() - t0; g_timing[4] = rounds; g_timing[5] = cand; g_timing[6] = bl; g_timing[7] = (double)exchanges;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// kao_solve_capped: cluster-wide per-broker load caps, priced (Lagrangian) over independent per-topic solves
// ------------------------------------------------------------------------------------------------
}  // extern "C"

// One run of the price loop at ONE price granularity F (price units per objective unit); kao_solve_capped below runs a portfolio of them.
static int capped_once(const kao_topic *topics, int32_t n_topics, const int32_t *replica_cap, const int32_t *devices, int32_t n_dev,
                       const kao_opts *opts, int32_t max_rounds, kao_result *results, int64_t *lagrangian_bound, const int F) {
    const double t0 = now_s();
    if (!topics || n_topics < 1 || !replica_cap || !results) return fail(KAO_ERR_INVALID, "null argument");
    const int B = topics[0].n_brokers;
    int wmax = 1;
    for (int i = 0; i < n_topics; ++i) {
        if (topics[i].n_brokers != B) return fail(KAO_ERR_INVALID, "kao_solve_capped: every topic must use the same broker set");
        if (topics[i].broker_w || topics[i].broker_wl) return fail(KAO_ERR_UNSUPPORTED, "kao_solve_capped: topics with their own broker weights");
        for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) wmax = std::max(wmax, topics[i].w[a][b]);
    }
    // Price granularity F (price units per objective unit).  Quarter units (F = 4: every role weight times 4 inside the per-topic
    // solves, prices in steps of 1/4) were tried in round 4 and tightened the Lagrangian bound of the medium golden (exact joint
    // optimum 9175: bound 9195 with whole prices, 9189 with quarters; the 12-topic case 4100 -> 4097 = exact) -- but K-search's
    // penalty range is tuned to the README's weights 1..4, with weights 4..16 per-topic solves came back infeasible and whole
    // rounds yielded no cap-respecting plan (round 4, GPU calls 13-15).  Round 5: the penalty range of the per-topic solves is scaled by
    // F as well (lam_min / lam_max times F: the ratio penalty : objective stays what K-search is tuned to) and the solves are
    // feasible again: medium golden bound 9195 (F = 1) -> 9178 (2) -> 9176 (4) against the exact 9175, the 12-topic case 4100 -> 4097 = exact.
    const int mu_max = std::min(1023, 4 * wmax * F);   // a price above every objective weight already repels every replica
    kao_opts o{};
    if (opts) o = *opts;
    const double limit = o.time_limit_s > 0 ? o.time_limit_s : 10.0;
    const int rounds = max_rounds > 0 ? max_rounds : 40;
    if (o.max_launches <= 0) o.max_launches = 6;
    if (F > 1) { o.lam_min = (o.lam_min > 0 ? o.lam_min : 1) * F; o.lam_max = (o.lam_max > 0 ? o.lam_max : 40) * F; }
    o.stop_at_bound = 1;
    o.target_objective = nullptr;
    std::vector<int32_t> mu((size_t)B, 0), bw((size_t)B, 0), mu_inc((size_t)B, 0);
    std::vector<kao_topic> tp(topics, topics + n_topics);
    for (int i = 0; i < n_topics; ++i)
        for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) tp[(size_t)i].w[a][b] = topics[i].w[a][b] * F;
    std::vector<std::vector<uint16_t>> buf((size_t)n_topics), inc((size_t)n_topics);
    std::vector<kao_result> res((size_t)n_topics), inc_res((size_t)n_topics);
    for (int i = 0; i < n_topics; ++i) buf[(size_t)i].assign((size_t)topics[i].n_partitions * topics[i].rf, (uint16_t)KAO_NONE);
    int64_t inc_total = -1, best_L = INT64_MAX, n_slots = 0;   // inc_total in objective units, best_L = floor(dual value in objective units)
    for (int i = 0; i < n_topics; ++i) n_slots += (int64_t)topics[i].n_partitions * topics[i].rf;
    std::vector<int64_t> load((size_t)B);
    auto floor_div = [](int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    // Rounds 0 .. rounds-1: WHOLE objective units (F price units), the loop of rounds 2-3.  Then up to rounds/2 more: with a
    // cap-respecting plan in hand, quarter units restarted from THAT plan's prices (with quarter steps from the start -- or from the
    // last prices -- the medium golden found no cap-respecting plan at all, and a toy lost two units: GPU calls 13 / 14); without
    // one, prices only rise (every broker over its cap, by its excess) until a plan respects the caps.
    int rc = KAO_OK, r = 0, fine_from = -1;
    bool raise_only = false;
    const int rounds_all = rounds + rounds / 2;
    for (; r < rounds_all; ++r) {
        const double left = limit - (now_s() - t0);
        if (r > 0 && left <= 0) break;
        if (r >= rounds && fine_from < 0 && !raise_only) {
            if (inc_total >= 0 && F > 1) { fine_from = r; mu = mu_inc; }
            else if (inc_total < 0) raise_only = true;
            else break;
        }
        int M = 0;
        for (int b = 0; b < B; ++b) M = std::max(M, mu[(size_t)b]);
        for (int b = 0; b < B; ++b) bw[(size_t)b] = M - mu[(size_t)b];   // weights must be >= 0: a constant M per replica does not change any argmax
        for (int i = 0; i < n_topics; ++i) {
            tp[(size_t)i].broker_w = M ? bw.data() : nullptr;
            res[(size_t)i] = kao_result{};
            res[(size_t)i].assignment = buf[(size_t)i].data();
        }
        o.time_limit_s = std::max(0.05, left / std::max(1, std::min(rounds_all - r, 8)));
        o.seed = (opts ? opts->seed : 0) + (uint64_t)r * 0x9E3779B97F4A7C15ull;
        rc = (devices && n_dev > 1) ? kao_solve_multi(tp.data(), n_topics, devices, n_dev, &o, res.data())
                                    : kao_solve(tp.data(), n_topics, &o, res.data());
        if (rc) break;
        // ---- broker loads over ALL topics (the allreduce(SUM) of a sharded deployment), objective without the weights ----
        std::fill(load.begin(), load.end(), 0);
        bool all_feasible = true;
        int64_t total = 0, total_w = 0;   // in 1/F units
        for (int i = 0; i < n_topics; ++i) {
            const kao_result &x = res[(size_t)i];
            if (x.status == KAO_STATUS_NO_FEASIBLE || x.status == KAO_STATUS_INFEASIBLE_PROVEN) { all_feasible = false; continue; }
            int64_t wsum = 0;
            for (size_t k = 0; k < buf[(size_t)i].size(); ++k) { const uint16_t b = buf[(size_t)i][k]; load[b]++; wsum += M ? bw[b] : 0; }
            total += x.objective - wsum;
            total_w += x.upper_bound;
        }
        int64_t worst = 0, priced = 0;
        for (int b = 0; b < B; ++b) {
            if (replica_cap[b] < 0) continue;
            worst = std::max<int64_t>(worst, load[(size_t)b] - replica_cap[b]);
            priced += (int64_t)mu[(size_t)b] * replica_cap[b];
        }
        // L(mu) <= sum of ANY valid per-topic upper bounds of the weighted topics - M * slots + mu . cap: round 3 -- K-bound now covers
        // weighted topics, so the per-topic bounds are (nearly) the weighted optima whether or not the search has met them
        if (all_feasible) best_L = std::min(best_L, floor_div(total_w - (int64_t)M * n_slots + priced, F));
        if (all_feasible && worst <= 0 && total / F > inc_total) {   // respects every cap: a candidate answer
            inc_total = total / F;
            mu_inc = mu;
            for (int i = 0; i < n_topics; ++i) {
                inc[(size_t)i] = buf[(size_t)i];
                inc_res[(size_t)i] = res[(size_t)i];
                int64_t wsum = 0;
                for (uint16_t b : buf[(size_t)i]) wsum += M ? bw[b] : 0;
                inc_res[(size_t)i].objective = (res[(size_t)i].objective - wsum) / F;
            }
        }
        if (inc_total >= 0 && best_L != INT64_MAX && inc_total >= best_L) break;   // incumbent meets the Lagrangian bound: optimal
        // ---- projected subgradient step on the prices, diminishing: alpha = 1 / (1 + r / 3) price units of the phase ----
        const bool fine = fine_from >= 0;
        const int rr = fine ? r - fine_from : (raise_only ? 0 : r);
        const int den = 1 + rr / 3;
        const int unit = fine ? 1 : F;
        if (raise_only && all_feasible && worst <= 0) break;   // the plan just booked respects every cap (loads are counted over feasible topics only: ADVICE r04)
        bool moved = false;
        for (int b = 0; b < B; ++b) {
            if (replica_cap[b] < 0) continue;
            const int64_t ex = load[(size_t)b] - replica_cap[b];
            int d = 0;
            if (ex > 0) d = unit * (int)std::max<int64_t>(1, ex / den);
            else if (ex < 0 && mu[(size_t)b] > 0 && !raise_only)
                d = -(int)std::min<int64_t>(mu[(size_t)b], unit * std::max<int64_t>(rr >= 6 ? 0 : 1, (-ex) / (2 * den)));
            const int nm = std::min(mu_max, std::max(0, mu[(size_t)b] + d));
            moved |= nm != mu[(size_t)b];
            mu[(size_t)b] = nm;
        }
        if (!moved) {   // prices are stationary: the coarse phase hands over (to the fine one or to raise-only), the others end
            if (fine || raise_only || r >= rounds - 1) break;
            r = rounds - 1;
        }
    }
    // ---- repair (round 4): one topic at a time from the incumbent plan.  Capped brokers that ended BELOW their cap were priced a
    // little too high for somebody: every topic in turn is solved again alone with those brokers one price unit cheaper (all
    // others as in the incumbent's round), and the new plan of that topic is taken when the topic's own objective grows and no
    // cap breaks.  Passes repeat while one of them gained and the clock allows.
    int repairs = 0;
    if (!rc && inc_total >= 0 && !(best_L != INT64_MAX && inc_total >= best_L)) {
        std::fill(load.begin(), load.end(), 0);
        for (int i = 0; i < n_topics; ++i) for (uint16_t b : inc[(size_t)i]) load[b]++;
        std::vector<int32_t> mu_t((size_t)B), bw_t((size_t)B);
        std::vector<uint16_t> one;
        bool gained = true;
        for (int pass = 0; pass < 4 && gained && !rc; ++pass) {
            gained = false;
            for (int i = 0; i < n_topics && !rc; ++i) {
                if (limit - (now_s() - t0) <= 0) break;
                bool any_slack = false;
                for (int b = 0; b < B; ++b) {
                    const bool slack = replica_cap[b] >= 0 && load[(size_t)b] < replica_cap[b] && mu_inc[(size_t)b] > 0;
                    mu_t[(size_t)b] = slack ? std::max(0, mu_inc[(size_t)b] - (pass % 2 ? 2 : 1)) : mu_inc[(size_t)b];
                    any_slack |= slack;
                }
                if (!any_slack) break;
                int M = 0;
                for (int b = 0; b < B; ++b) M = std::max(M, mu_t[(size_t)b]);
                for (int b = 0; b < B; ++b) bw_t[(size_t)b] = M - mu_t[(size_t)b];
                kao_topic t1 = tp[(size_t)i];
                t1.broker_w = M ? bw_t.data() : nullptr;
                one.assign(inc[(size_t)i].size(), (uint16_t)KAO_NONE);
                kao_result r1{};
                r1.assignment = one.data();
                o.time_limit_s = std::max(0.02, std::min(0.25, limit - (now_s() - t0)));
                o.seed = (opts ? opts->seed : 0) + 0xD1B54A32D192ED03ull * (uint64_t)(pass * n_topics + i + 1);
                rc = kao_solve(&t1, 1, &o, &r1);
                if (rc) break;
                if (r1.status == KAO_STATUS_NO_FEASIBLE || r1.status == KAO_STATUS_INFEASIBLE_PROVEN) continue;
                int64_t wsum = 0;
                for (uint16_t b : one) wsum += M ? bw_t[b] : 0;
                const int64_t obj1 = (r1.objective - wsum) / F;
                if (obj1 <= inc_res[(size_t)i].objective) continue;
                bool ok = true;
                for (uint16_t b : inc[(size_t)i]) load[b]--;
                for (uint16_t b : one) load[b]++;
                for (int b = 0; b < B && ok; ++b) ok = replica_cap[b] < 0 || load[(size_t)b] <= replica_cap[b];
                if (!ok) {
                    for (uint16_t b : one) load[b]--;
                    for (uint16_t b : inc[(size_t)i]) load[b]++;
                    continue;
                }
                inc_total += obj1 - inc_res[(size_t)i].objective;
                inc[(size_t)i] = one;
                inc_res[(size_t)i] = r1;
                inc_res[(size_t)i].objective = obj1;
                gained = true;
                ++repairs;
            }
        }
    }
    if (!rc) {
        for (int i = 0; i < n_topics; ++i) {
            uint16_t *dst = results[i].assignment;
            if (inc_total >= 0) {
                results[i] = inc_res[(size_t)i];
                results[i].status = (best_L != INT64_MAX && inc_total >= best_L) ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
                results[i].upper_bound = best_L != INT64_MAX ? best_L : INT64_MAX;   // a bound on the SUM over all topics
                if (dst) std::memcpy(dst, inc[(size_t)i].data(), inc[(size_t)i].size() * 2);
            } else {
                results[i] = res[(size_t)i];
                results[i].status = KAO_STATUS_NO_FEASIBLE; results[i].objective = -1;
            }
            results[i].assignment = dst;
        }
        if (lagrangian_bound) *lagrangian_bound = best_L;
    }
    g_timing[3] = now_s() - t0; g_timing[4] = r; (void)repairs;
    return rc;
}

extern "C" {

// A portfolio over the price granularity (round 5): quarter units give the tightest Lagrangian bound (and prices between the whole
// units, which is where the exact joint optimum's prices often lie), half and whole units different plans -- which granularity finds
// the best cap-respecting plan varies by instance (medium golden: plan 9169 / 9175 / 9169 with F = 4 / 2 / 1, the 12-topic case 4095 /
// 4093 / 4097).  The runs share the time limit; the best plan and the smallest bound of all runs are returned, and the portfolio ends as
// soon as they meet.
int kao_solve_capped(const kao_topic *topics, int32_t n_topics, const int32_t *replica_cap, const int32_t *devices, int32_t n_dev,
                     const kao_opts *opts, int32_t max_rounds, kao_result *results, int64_t *lagrangian_bound) {
    const double t0 = now_s();
    if (!topics || n_topics < 1 || !replica_cap || !results) return fail(KAO_ERR_INVALID, "null argument");
    int wmax = 1;
    for (int i = 0; i < n_topics; ++i) for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) wmax = std::max(wmax, topics[i].w[a][b]);
    std::vector<int> fs;
    for (int f : {4, 2, 1}) if (f == 1 || wmax * f <= 255) fs.push_back(f);   // F = 1 always runs (weights up to 1023 are valid; only the scaled runs need room)
    kao_opts o{};
    if (opts) o = *opts;
    const double limit = o.time_limit_s > 0 ? o.time_limit_s : 10.0;
    std::vector<std::vector<uint16_t>> buf((size_t)n_topics);
    std::vector<kao_result> res((size_t)n_topics);
    for (int i = 0; i < n_topics; ++i) buf[(size_t)i].assign((size_t)topics[i].n_partitions * topics[i].rf, (uint16_t)KAO_NONE);
    int64_t best_total = -1, best_L = INT64_MAX;
    int rc = KAO_OK;
    double rounds_total = 0;
    auto copy_out = [&]() {
        for (int i = 0; i < n_topics; ++i) {
            uint16_t *dst = results[i].assignment;
            results[i] = res[(size_t)i];
            results[i].assignment = dst;
            if (dst) std::memcpy(dst, buf[(size_t)i].data(), buf[(size_t)i].size() * 2);
        }
    };
    for (size_t k = 0; k < fs.size() && !rc; ++k) {
        const double left = limit - (now_s() - t0);
        if (k > 0 && left <= 0.05) break;
        for (int i = 0; i < n_topics; ++i) { res[(size_t)i] = kao_result{}; res[(size_t)i].assignment = buf[(size_t)i].data(); }
        o.time_limit_s = std::max(0.05, left / (double)(fs.size() - k));
        int64_t L = INT64_MAX;
        rc = capped_once(topics, n_topics, replica_cap, devices, n_dev, &o, max_rounds, res.data(), &L, fs[k]);
        if (rc) break;
        rounds_total += g_timing[4];
        best_L = std::min(best_L, L);
        int64_t total = 0;
        bool ok = true;
        for (int i = 0; i < n_topics; ++i) { ok = ok && res[(size_t)i].status != KAO_STATUS_NO_FEASIBLE; total += res[(size_t)i].objective; }
        if ((ok && total > best_total) || best_total < 0) {   // (no cap-respecting plan yet: the last run's report -- NO_FEASIBLE -- stands until one is found)
            if (ok) best_total = total;
            copy_out();
        }
        if (best_total >= 0 && best_L != INT64_MAX && best_total >= best_L) break;
    }
    if (!rc) {
        for (int i = 0; i < n_topics && best_total >= 0; ++i) {
            results[i].status = (best_L != INT64_MAX && best_total >= best_L) ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
            results[i].upper_bound = best_L;
        }
        if (lagrangian_bound) *lagrangian_bound = best_L;
    }
    g_timing[3] = now_s() - t0; g_timing[4] = rounds_total;
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// ONE LP over several devices (round 6): the collective side of kao_lp.hip's shards, and a test hook
// ------------------------------------------------------------------------------------------------
namespace {
// Every shard's host thread walks the same sequence of launches; where the sequence holds a collective each thread hands in its buffer
// and stream and waits; the LAST one to arrive issues the grouped ncclAllReduce(ncclDouble, ncclSum | ncclMin) for every rank -- the
// single-process, one-thread-per-group calling pattern kao_solve_multi's elite exchange uses, served by RCCL on distinct devices and by
// the loop-back table on logical shards -- and releases the others.  A thread that fails raises `failed`: nobody waits for it.
struct LpGroup : LpColl {
    int n = 0;
    std::vector<ncclComm_t> comms;
    const Rccl *api = nullptr;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0, rc = KAO_OK;
    uint64_t gen = 0, collectives = 0;
    bool failed = false;
    struct Op { double *buf; size_t n; bool is_min; hipStream_t st; };
    std::vector<Op> ops;
    int issue() {
        for (int r = 1; r < n; ++r)
            if (ops[(size_t)r].n != ops[0].n || ops[(size_t)r].is_min != ops[0].is_min) return fail(KAO_ERR_HIP, "KAO-LP shards: the ranks disagree about a collective");
        ncclResult_t nr = api->GroupStart();
        for (int r = 0; r < n && nr == ncclSuccess; ++r) {
            const Op &o = ops[(size_t)r];
            nr = api->AllReduce(o.buf, o.buf, o.n, ncclDouble, o.is_min ? ncclMin : ncclSum, comms[(size_t)r], o.st);
        }
        if (nr == ncclSuccess) nr = api->GroupEnd();
        ++collectives;
        return nr == ncclSuccess ? KAO_OK : fail(KAO_ERR_HIP, std::string("KAO-LP shards: all-reduce: ") + api->GetErrorString(nr));
    }
    int allreduce(int rank, double *buf, size_t cnt, bool is_min, void *stream) override {
        std::unique_lock<std::mutex> lk(mu);
        if (failed) return rc ? rc : KAO_ERR_HIP;
        ops[(size_t)rank] = Op{buf, cnt, is_min, static_cast<hipStream_t>(stream)};
        const uint64_t my = gen;
        if (++arrived == n) {
            const int r = issue();
            arrived = 0; ++gen;
            if (r) { failed = true; rc = r; }
            cv.notify_all();
            return r;
        }
        cv.wait(lk, [&] { return gen != my || failed; });
        return failed ? (rc ? rc : KAO_ERR_HIP) : KAO_OK;
    }
    void give_up(int code) { std::lock_guard<std::mutex> lk(mu); if (!failed) { failed = true; rc = code; } cv.notify_all(); }
};

// N shard contexts behind ONE LpCtx-shaped front (kao_internal.h LpFan): one persistent host thread per shard (its device current, the
// collectives of LpGroup between them); a call of the front runs the same lp_* function on every shard's thread and returns when all have
// ENQUEUED their part.  Marks are read from shard 0 (the scalars are replicated); an abort reaches every shard.
struct LpFanImpl : LpFan {
    const kao_topic *t = nullptr;
    std::vector<int> devs, p0s;
    LpGroup group;
    std::vector<LpCtx *> ctx;
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    std::function<int(int)> job;
    uint64_t job_gen = 0;
    int pending = 0;
    std::vector<int> rcs;
    bool quit = false;
    void worker(int r) {
        t_device = devs[(size_t)r];
        (void)hipSetDevice(t_device);
        t_lp_inner = true;
        uint64_t seen = 0;
        for (;;) {
            std::function<int(int)> f;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return quit || job_gen != seen; });
                if (quit) return;
                seen = job_gen; f = job;
            }
            const int e = f(r);
            if (e) group.give_up(e);
            std::lock_guard<std::mutex> lk(mu);
            rcs[(size_t)r] = e;
            if (--pending == 0) cv_done.notify_all();
        }
    }
    int run(std::function<int(int)> f) {     // f(rank) on every shard's thread; first failure
        std::unique_lock<std::mutex> lk(mu);
        job = std::move(f); ++job_gen; pending = (int)devs.size();
        std::fill(rcs.begin(), rcs.end(), KAO_OK);
        cv_go.notify_all();
        cv_done.wait(lk, [&] { return pending == 0; });
        for (int e : rcs) if (e) return e;
        return KAO_OK;
    }
    int open(const kao_topic *topic, const int *devices, int n) {
        t = topic;
        devs.assign(devices, devices + n);
        group.n = n; group.ops.resize((size_t)n);
        int rc = comms_for(devs, group.comms, &group.api);
        if (rc) return rc;
        p0s.resize((size_t)n + 1);
        for (int r = 0; r <= n; ++r) p0s[(size_t)r] = (int)((int64_t)t->n_partitions * r / n);
        ctx.assign((size_t)n, nullptr); rcs.assign((size_t)n, KAO_OK);
        for (int r = 0; r < n; ++r) th.emplace_back(&LpFanImpl::worker, this, r);
        return run([&](int r) { LpShard sh{p0s[(size_t)r], p0s[(size_t)r + 1], r, &group}; return lp_open(t, &ctx[(size_t)r], &sh); });
    }
    int begin(double tol, int maxit, double pert, uint32_t salt) override { return run([&](int r) { return lp_begin(ctx[(size_t)r], tol, maxit, pert, salt); }); }
    int enqueue_mark(int k, int slot) override { return run([&](int r) { return lp_enqueue_mark(ctx[(size_t)r], k, slot); }); }
    struct Inner { bool saved; Inner() : saved(t_lp_inner) { t_lp_inner = true; } ~Inner() { t_lp_inner = saved; } };
    int poll_mark(int slot, int *status, int *iterations, double deadline) override {
        Inner in;
        int st = 0, it = 0;
        const int rc = lp_poll_mark(ctx[0], slot, &st, &it, deadline);
        if (!rc && st == 4) for (size_t r = 1; r < ctx.size(); ++r) lp_abort(ctx[r]);     // the deadline passed: shard 0 raised its flag, the others follow
        if (status) *status = st;
        if (iterations) *iterations = it;
        if (cur_device() >= 0) (void)hipSetDevice(cur_device());
        return rc;
    }
    int finish(int32_t *multipliers, double stats[8], double *trace) override {
        return run([&](int r) { return lp_finish(ctx[(size_t)r], r == 0 ? multipliers : nullptr, r == 0 ? stats : nullptr, r == 0 ? trace : nullptr); });
    }
    int primal(uint8_t *q, int32_t *zq) override {     // the shards' quantised rows side by side
        const int P = t->n_partitions, K = 2 * t->rf_cur + 2 * t->n_racks;
        std::vector<std::vector<uint8_t>> qs(ctx.size());
        std::vector<std::vector<int32_t>> zs(ctx.size(), std::vector<int32_t>(2 * (size_t)t->n_brokers));
        const int rc = run([&](int r) { qs[(size_t)r].resize((size_t)K * (size_t)(p0s[(size_t)r + 1] - p0s[(size_t)r])); return lp_primal(ctx[(size_t)r], qs[(size_t)r].data(), zs[(size_t)r].data()); });
        if (rc) return rc;
        for (size_t r = 0; r < ctx.size(); ++r) {
            const int pa = p0s[r], pn = p0s[r + 1] - pa;
            for (int k = 0; k < K; ++k) std::memcpy(q + (size_t)k * P + pa, qs[r].data() + (size_t)k * pn, (size_t)pn);
        }
        std::memcpy(zq, zs[0].data(), zs[0].size() * 4);
        return KAO_OK;
    }
    void abort() override { Inner in; for (LpCtx *c : ctx) if (c) lp_abort(c); if (cur_device() >= 0) (void)hipSetDevice(cur_device()); }
    void shutdown() {
        if (!th.empty()) {
            (void)run([&](int r) { if (ctx[(size_t)r]) { lp_abort(ctx[(size_t)r]); lp_close(ctx[(size_t)r]); ctx[(size_t)r] = nullptr; } return KAO_OK; });
            { std::lock_guard<std::mutex> lk(mu); quit = true; }
            cv_go.notify_all();
            for (std::thread &x : th) x.join();
            th.clear();
        }
        if (cur_device() >= 0) (void)hipSetDevice(cur_device());
    }
    void close() override { shutdown(); delete this; }
    ~LpFanImpl() override { shutdown(); }
};
}  // namespace

int kao::lp_open_fan(const kao_topic *t, const int *devices, int n_dev, LpCtx **out) {
    LpFanImpl *f = new LpFanImpl();
    const int rc = f->open(t, devices, n_dev);
    if (rc) { delete f; return rc; }
    lp_set_fan(f->ctx[0], f);
    *out = f->ctx[0];
    return KAO_OK;
}

extern "C" {

// Test hook (include/kao.h): the LP of ONE topic solved by n_dev shards (contiguous partition ranges; devices may repeat with
// KAO_RCCL_LOOPBACK=1: logical shards), then the same certificate evaluation and rounding as kao_lp_bound / kao_lp_round.
int kao_lp_sharded_test(const kao_topic *t, const int32_t *devices, int32_t n_dev, double pert, uint32_t salt, double tol, int32_t max_iters,
                        int64_t *bound, uint16_t *assignment, int64_t *objective, int32_t violations[8], double stats[8]) {
    if (!t || !devices || n_dev < 1 || n_dev > kMaxDevices) return fail(KAO_ERR_INVALID, "kao_lp_sharded_test: bad arguments");
    int rc = require_init();
    if (rc) return rc;
    if ((rc = validate(t))) return rc;
    if (t->n_partitions < n_dev) return fail(KAO_ERR_INVALID, "kao_lp_sharded_test: fewer partitions than shards");
    std::vector<int> devs(devices, devices + n_dev);
    bool distinct = true;
    for (int i = 0; i < n_dev; ++i) for (int j = 0; j < i; ++j) distinct &= devs[(size_t)i] != devs[(size_t)j];
    if (!distinct && !loopback_wanted()) return fail(KAO_ERR_INVALID, "kao_lp_sharded_test: repeated devices are logical shards: set KAO_RCCL_LOOPBACK=1");
    LpGroup g;
    g.n = n_dev; g.ops.resize((size_t)n_dev);
    if ((rc = comms_for(devs, g.comms, &g.api))) return rc;
    const int P = t->n_partitions, K = 2 * t->rf_cur + 2 * t->n_racks;
    std::vector<LpCtx *> ctx((size_t)n_dev, nullptr);
    std::vector<int> rcs((size_t)n_dev, KAO_OK), p0s((size_t)n_dev + 1, 0);
    for (int r = 0; r <= n_dev; ++r) p0s[(size_t)r] = (int)((int64_t)P * r / n_dev);
    std::vector<std::vector<uint8_t>> qs((size_t)n_dev);
    std::vector<int32_t> zq(2 * (size_t)t->n_brokers), mult(2 * (size_t)t->n_brokers + (size_t)t->n_racks);
    double st8[8] = {0};
    const double eps = pert > 0 ? pert : (pert < 0 ? 0.0 : lp_default_pert(t));       // pert < 0: the model's own LP (certificate only)
    const double t0 = now_s();
    auto work = [&](int r) {
        t_device = devs[(size_t)r];
        int e = hipSetDevice(t_device) == hipSuccess ? KAO_OK : fail(KAO_ERR_NO_DEVICE, "hipSetDevice");
        LpShard sh{p0s[(size_t)r], p0s[(size_t)r + 1], r, &g};
        if (!e) e = lp_open(t, &ctx[(size_t)r], &sh);
        double stl[8] = {0};
        if (!e) e = lp_solve(ctx[(size_t)r], tol > 0 ? tol : 1e-8, max_iters > 0 ? max_iters : 150, r == 0 ? mult.data() : nullptr, stl, nullptr, eps, salt);
        if (!e) {
            qs[(size_t)r].resize((size_t)K * (size_t)(p0s[(size_t)r + 1] - p0s[(size_t)r]));
            std::vector<int32_t> zl(2 * (size_t)t->n_brokers);
            e = lp_primal(ctx[(size_t)r], qs[(size_t)r].data(), zl.data());
            if (!e && r == 0) { zq = zl; std::memcpy(st8, stl, sizeof stl); }
        }
        if (e) g.give_up(e);
        rcs[(size_t)r] = e;
    };
    {
        std::vector<std::thread> th;
        for (int r = 1; r < n_dev; ++r) th.emplace_back(work, r);
        const int saved = t_device;
        work(0);
        for (std::thread &x : th) x.join();
        t_device = saved;
        if (cur_device() >= 0) (void)hipSetDevice(cur_device());
    }
    for (LpCtx *c : ctx) if (c) lp_close(c);
    for (int e : rcs) if (e) return e;
    const double t_lp = now_s();
    // the shards' quantised iterates side by side: row k of the whole topic = the shards' rows k, in partition order
    std::vector<uint8_t> q((size_t)K * P);
    for (int r = 0; r < n_dev; ++r) {
        const int pa = p0s[(size_t)r], pn = p0s[(size_t)r + 1] - pa;
        for (int k = 0; k < K; ++k) std::memcpy(q.data() + (size_t)k * P + pa, qs[(size_t)r].data() + (size_t)k * pn, (size_t)pn);
    }
    if (bound) {   // the dual value at the shards' common multipliers, in integers: one K-bound iteration from them (as kao_lp_bound)
        kao_opts o{};
        o.restarts = kWaves;
        kao_session *s = nullptr;
        if ((rc = kao_session_create(t, 1, &o, &s))) return rc;
        if (!s->dual_ok[0]) { kao_session_destroy(s); return fail(KAO_ERR_UNSUPPORTED, "topic outside K-bound's limits"); }
        rc = kao_session_set_dual_state(s, 0, mult.data(), mult.data() + t->n_brokers, mult.data() + 2 * (size_t)t->n_brokers);
        const int64_t target = 0;
        int32_t fl = 0, itn = 0;
        int64_t bd = 0;
        if (!rc) rc = kao_session_bound_step(s, &target, 1);
        if (!rc) rc = kao_session_bounds(s, nullptr, &fl, &itn);
        if (!rc) rc = kao_session_dual_state(s, 0, nullptr, nullptr, nullptr, &bd);
        if (!rc) *bound = (fl & 4) || itn == 0 ? INT64_MAX : (bd >= 0 ? bd / kDualScale : -((-bd + kDualScale - 1) / kDualScale));
        kao_session_destroy(s);
        if (rc) return rc;
    }
    int32_t rep[4] = {0, 0, 0, 0};
    if (assignment) {
        if ((rc = lp_round_assignment(t, q.data(), zq.data(), nullptr, assignment, rep))) return rc;
        int64_t obj = 0;
        int32_t viol[8] = {0};
        if ((rc = kao_evaluate(t, assignment, &obj, viol))) return rc;
        if (objective) *objective = obj;
        if (violations) std::memcpy(violations, viol, sizeof viol);
    }
    if (stats) { stats[0] = st8[0]; stats[1] = st8[3]; stats[2] = rep[0]; stats[3] = (double)g.collectives; stats[4] = st8[2]; stats[5] = (t_lp - t0) * 1e3; stats[6] = (now_s() - t_lp) * 1e3; stats[7] = eps; }
    return KAO_OK;
}

int kao_rccl_loopback_counts(uint64_t out[2]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    out[0] = g_loop_allreduces; out[1] = g_loop_broadcasts;
    return KAO_OK;
}

int kao_last_solve_lp(double out[8]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    for (int i = 0; i < 8; ++i) out[i] = g_lp[i];
    return KAO_OK;
}
int kao_last_solve_timing(double out[16]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    for (int i = 0; i < 16; ++i) out[i] = g_timing[i];
    return KAO_OK;
}

int kao_last_solve_profile(double out[8]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    for (int i = 0; i < 8; ++i) out[i] = g_profile[i];
    return KAO_OK;
}

}  // extern "C"
