// kao_solve.cpp -- host side of libkao.so (see kao_host.h): the solve loops on top of sessions.
//   kao_solve         one device: K-search launches, K-bound beside them on its own stream, KAO-CX (kao_cycle.hip) for
//                     incumbents the search has stopped improving, stop at the proof
//   kao_solve_multi   several GPUs in one process: topics dealt LPT, or every GPU on every topic with the elites exchanged by
//                     ncclAllReduce(min) / ncclBroadcast on the resident key buffers (librccl is opened on first use)
#include <cstdio>
#include <cstring>

#include "kao_rccl.h"

namespace kao {
thread_local SolveCounters g_last{};   // this thread's last solve (kao_host.h); kao_capped.cpp adds its rounds
}  // namespace kao

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
                hbm = hbm || (int64_t)t.n_partitions * nw * 4 + 8 * 1024 > kLdsLimit;
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

// The counters of the last solve (kao_host.h g_last) that are summed over its runs start from zero in every call (kao_solve_multi's kept the previous kao_solve's values)
void clear_run_counters() {
    SolveTiming &t = g_last.timing;
    t.time_to_best = t.delta_candidates = t.bound_launches = t.elite_exchanges = t.bound_iters = t.cx_calls = t.cx_gains = t.search_iters = 0;
    t.generations = t.cx_further_starts = t.lp_solves = t.lp_iters = 0;
    g_last.lp = SolveLp{};
}
// A finished run's counters, added into the record: kao_solve calls this once, kao_solve_multi once per device (KAO-LP over all devices: a
// replicated topic in the LP's regime is a race, every device runs its own solve)
void add_run_counters(const SolveRun &run) {
    SolveTiming &t = g_last.timing;
    t.time_to_best = std::max(t.time_to_best, run.t_last_improve);
    t.delta_candidates += (double)run.s->delta_total; t.bound_launches += (double)run.s->bound_launches;
    for (int32_t v : run.s->dual_iters) t.bound_iters += (double)v;   // K-bound iterations, summed over the topics
    t.cx_calls += run.cx_calls; t.cx_gains += run.cx_gains; t.search_iters += (double)run.iters_done; t.generations += run.generations;
    t.cx_further_starts += run.cx_more; t.lp_solves += run.lp_solves; t.lp_iters += run.lp_iters;
    SolveLp &l = g_last.lp;
    l.solves += run.lp_solves; l.iterations += run.lp_iters; l.rounded += run.lp_rounded; l.adopted += run.lp_round_adopted; l.fractional_partitions += run.lp_round_fractional;
}

// ---- kao_solve_multi: one process, several GPUs -- the pieces of the function below ----
// One device's share of the job.  `run` closes its KAO-CX / KAO-LP contexts and its session when it goes, on every way out of
// kao_solve_multi: the destructor's body (which runs before the members') makes the device current for that.
struct Dev {
    SolveRun run; std::vector<kao_topic> tp; std::vector<kao_result> res; std::vector<int64_t> tgt;
    DeviceScope *scope = nullptr; int device = -1;   // set once the run is about to begin
    ~Dev() { if (scope) (void)scope->to(device); }
};

int check_multi_args(const kao_topic *topics, int32_t n_topics, const int32_t *devices, int32_t n_dev, const kao_opts *opts, const kao_result *results, std::vector<int> &devs, bool &distinct) {
    if (!topics || n_topics < 1 || !results) return fail(KAO_ERR_INVALID, "no topics / null results");
    if (!devices || n_dev < 1 || n_dev > kMaxDevices) return fail(KAO_ERR_INVALID, "bad device list");
    if (opts && (opts->team < 0 || opts->team > kTeamMax || opts->schedule < 0 || opts->schedule > 1)) return fail(KAO_ERR_INVALID, "kao_opts: team must be 0..8, schedule 0 or 1");
    int n_hw = 0;
    if (hipGetDeviceCount(&n_hw) != hipSuccess || n_hw <= 0) return fail(KAO_ERR_NO_DEVICE, "no HIP device");
    devs.assign(devices, devices + n_dev);
    distinct = true;
    for (int i = 0; i < n_dev; ++i) {
        if (devs[(size_t)i] < 0 || devs[(size_t)i] >= n_hw) return fail(KAO_ERR_INVALID, "device ordinal out of range");
        for (int j = 0; j < i; ++j) distinct &= devs[(size_t)j] != devs[(size_t)i];
    }
    return KAO_OK;
}

// ---- shards: LPT by brokers x partitions (independent sub-problems, README.md:146-184); replicated: every device gets every topic ----
std::vector<std::vector<int>> assign_shards(const kao_topic *topics, int n_topics, int n_dev, bool replicated) {
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
    return shard;
}

// certificates: any GPU's bound is valid for the topic
void share_certificates(std::vector<Dev> &D, int n_topics) {
    for (int i = 0; i < n_topics; ++i) {
        int64_t ub = INT64_MAX;
        for (Dev &x : D) ub = std::min(ub, x.run.s->ub[(size_t)i]);
        for (Dev &x : D) x.run.s->ub[(size_t)i] = ub;
    }
}

// ---- elite exchange: per topic the smallest packed key of all devices and the device that holds it (true: some device's incumbent is not the global one) ...
bool global_best_keys(const std::vector<Dev> &D, int n_topics, std::vector<uint64_t> &gmin, std::vector<int> &root) {
    const int n_dev = (int)D.size();
    bool differ = false;
    for (int i = 0; i < n_topics; ++i) {
        gmin[(size_t)i] = ~0ull; root[(size_t)i] = 0;
        for (int d = 0; d < n_dev; ++d) {
            const uint64_t k = D[(size_t)d].run.keys[(size_t)i] | 0;  // host copy read by after_launch
            if (k < gmin[(size_t)i]) { gmin[(size_t)i] = k; root[(size_t)i] = d; }
        }
        for (int d = 0; d < n_dev; ++d) differ |= (D[(size_t)d].run.keys[(size_t)i] >> 20) != (gmin[(size_t)i] >> 20);
    }
    return differ;
}
// ... then min-allreduce of the keys on the resident buffers, winners broadcast: stages every GPU's current winners, moves the global ones to every GPU (`api`: the table of the communicators `comms`, or null: logical
// shards on one device without KAO_RCCL_LOOPBACK=1), and has every GPU adopt them
int exchange_elites(std::vector<Dev> &D, int n_topics, const std::vector<uint64_t> &gmin, const std::vector<int> &root, const Rccl *api, const std::vector<ncclComm_t> &comms) {
    const int n_dev = (int)D.size();
    int rc = KAO_OK;
    for (int d = 0; d < n_dev && !rc; ++d) {   // stage every GPU's current winners
        kao_session *s = D[(size_t)d].run.s;
        if (hipSetDevice(s->device) != hipSuccess) { rc = fail(KAO_ERR_HIP, "hipSetDevice"); break; }
        launch_gather(s->d_topics, s->n_topics, s->d_keys, s->d_best, s->d_viol, s->d_win_assign, s->d_win_viol, s->stream);
    }
    if (!rc && api) {
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
    return rc;
}

// every device's results read back under its own device: dealt topics go to their places; of replicated ones the GPU holding the best key answers
int collect_results(std::vector<Dev> &D, DeviceScope &scope, const std::vector<int> &devs, const std::vector<std::vector<int>> &shard, bool replicated,
                    const kao_topic *topics, int n_topics, bool hit_time, kao_result *results) {
    const int n_dev = (int)D.size();
    int rc = KAO_OK;
    for (int d = 0; d < n_dev && !rc && !replicated; ++d) {
        Dev &x = D[(size_t)d];
        if (!x.run.s) continue;
        x.res.assign(x.tp.size(), kao_result{});
        for (size_t k = 0; k < x.tp.size(); ++k) x.res[k].assignment = results[shard[(size_t)d][k]].assignment;
        if (!(rc = scope.to(devs[(size_t)d]))) rc = x.run.finish(x.res.data(), hit_time);
        for (size_t k = 0; k < x.tp.size() && !rc; ++k) results[shard[(size_t)d][k]] = x.res[k];
    }
    if (!replicated) return rc;
    std::vector<std::vector<kao_result>> rs((size_t)n_dev, std::vector<kao_result>((size_t)n_topics));
    std::vector<std::vector<std::vector<uint16_t>>> bufs((size_t)n_dev);
    for (int d = 0; d < n_dev && !rc; ++d) {
        bufs[(size_t)d].resize((size_t)n_topics);
        for (int i = 0; i < n_topics; ++i) {
            bufs[(size_t)d][(size_t)i].assign((size_t)topics[i].n_partitions * topics[i].rf, (uint16_t)KAO_NONE);
            rs[(size_t)d][(size_t)i] = kao_result{};
            rs[(size_t)d][(size_t)i].assignment = bufs[(size_t)d][(size_t)i].data();
        }
        if (!(rc = scope.to(devs[(size_t)d]))) rc = D[(size_t)d].run.finish(rs[(size_t)d].data(), hit_time);
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
    return rc;
}

}  // namespace

extern "C" {
int kao_solve(const kao_topic *topics, int32_t n_topics, const kao_opts *opts, kao_result *results) {
    const double t0 = now_s();
    if (!results) return fail(KAO_ERR_INVALID, "null results");
    if (opts && (opts->team < 0 || opts->team > kTeamMax || opts->schedule < 0 || opts->schedule > 1)) return fail(KAO_ERR_INVALID, "kao_opts: team must be 0..8, schedule 0 or 1");
    const kao_opts so = solve_defaults(topics, n_topics, opts);
    SolveRun run;
    int rc = run.begin(topics, n_topics, so, opts ? opts->target_objective : nullptr, t0, true, true);
    if (rc) return rc;
    SolveTiming &tm = g_last.timing;
    tm.session_ready = now_s() - t0;
    const kao_opts &o = run.s->opts;
    bool hit_time = false;
    for (;;) {
        if ((rc = run.launch()) || (rc = run.after_launch())) return rc;
        if (o.stop_at_bound && run.all_done) break;
        if (o.max_launches > 0 && run.launches >= o.max_launches) break;
        if (now_s() - t0 >= o.time_limit_s) { hit_time = true; break; }
    }
    rc = run.finish(results, hit_time);
    tm.results_read_back = now_s() - t0;
    clear_run_counters();   // (elite exchanges between GPUs: none on one device)
    add_run_counters(run);
    g_last.profile = SolveProfile{};
    if (o.profile) {
        kao_stats st{};
        if (kao_session_stats(run.s, &st) == KAO_OK)
            g_last.profile = SolveProfile{st.ms_search, st.ms_eval, (double)st.launches, (double)st.n_restarts_total, (double)st.search_bytes_algo,
                                          (double)st.delta_candidates, (double)st.lds_bytes_search, (double)st.blocks_search};
    }
    kao_session_destroy(run.s);
    run.s = nullptr;
    tm.returned = now_s() - t0; tm.launches = run.launches;
    return rc;
}

int kao_solve_multi(const kao_topic *topics, int32_t n_topics, const int32_t *devices, int32_t n_dev, const kao_opts *opts,
                    kao_result *results) {
    const double t0 = now_s();
    std::vector<int> devs;
    bool distinct = true;
    int rc = check_multi_args(topics, n_topics, devices, n_dev, opts, results, devs, distinct);
    if (rc || (!is_init() && (rc = kao_init(devs[0])))) return rc;
    if (n_dev == 1) {   // a list of one device: exactly kao_solve (generations, islands), on THAT device (callers used to
                        // fall back to the kao_init device and ignore the ordinal they had been given)
        DeviceScope on(devs[0]);
        return kao_solve(topics, n_topics, opts, results);
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
    const std::vector<std::vector<int>> shard = assign_shards(topics, n_topics, n_dev, replicated);
    std::vector<ncclComm_t> comms;
    // logical shards on one device (tests) merge through plain copies -- or, with KAO_RCCL_LOOPBACK=1, through the same grouped
    // collective calls as distinct devices, served by the in-process loop-back table
    const Rccl *api = nullptr;
    if (replicated && (distinct || loopback_wanted()) && (rc = comms_for(devs, comms, &api))) return rc;
    DeviceScope scope;   // the caller's device comes back AFTER the devices' runs are gone (D is declared below it), on every return
    std::vector<Dev> D((size_t)n_dev);
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
        x.scope = &scope; x.device = devs[(size_t)d];
        if ((rc = scope.to(x.device))) break;
        rc = x.run.begin(x.tp.data(), (int)x.tp.size(), o, x.tgt.empty() ? nullptr : x.tgt.data(), t0);
    }
    if (rc) return rc;
    SolveTiming &tm = g_last.timing;
    tm.session_ready = now_s() - t0;
    const int exch = std::max(1, so.elite_period);
    bool hit_time = false;
    int rounds = 0;
    uint64_t exchanges = 0;
    std::vector<uint64_t> gmin((size_t)n_topics);
    std::vector<int> root((size_t)n_topics);
    for (;;) {
        if (shard_lp && D[0].run.s) lp_pause = D[0].run.search_paused();
        for (int d = 0; d < n_dev && !rc; ++d) if (D[(size_t)d].run.s && !(rc = scope.to(devs[(size_t)d]))) rc = D[(size_t)d].run.launch();
        for (int d = 0; d < n_dev && !rc; ++d) if (D[(size_t)d].run.s && !(rc = scope.to(devs[(size_t)d]))) rc = D[(size_t)d].run.after_launch();
        if (rc) break;
        ++rounds;
        if (replicated) {
            share_certificates(D, n_topics);
            if (rounds % exch == 0 || so.stop_at_bound) {
                const bool differ = global_best_keys(D, n_topics, gmin, root);
                if (differ && rounds % exch == 0) {
                    ++exchanges;
                    if ((rc = exchange_elites(D, n_topics, gmin, root, api, comms))) break;
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
    if (!rc) rc = collect_results(D, scope, devs, shard, replicated, topics, n_topics, hit_time, results);
    tm.results_read_back = now_s() - t0;
    clear_run_counters();   // counters of this call, summed over the devices
    for (Dev &x : D) if (x.run.s) add_run_counters(x.run);
    tm.elite_exchanges = (double)exchanges;
    for (int d = 0; d < n_dev; ++d) if (D[(size_t)d].run.s) { (void)scope.to(devs[(size_t)d]); kao_session_destroy(D[(size_t)d].run.s); D[(size_t)d].run.s = nullptr; }
    tm.returned = now_s() - t0; tm.launches = rounds;
    return rc;
}

// The array layouts of include/kao.h: here and nowhere else.
int kao_last_solve_lp(double out[8]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    const SolveLp &l = g_last.lp;
    const double v[8] = {l.solves, l.iterations, l.rounded, l.adopted, l.fractional_partitions, 0, 0, 0};
    std::copy(v, v + 8, out);
    return KAO_OK;
}
int kao_last_solve_timing(double out[16]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    const SolveTiming &t = g_last.timing;
    const double v[16] = {t.session_ready, t.time_to_best, t.results_read_back, t.returned, t.launches, t.delta_candidates, t.bound_launches, t.elite_exchanges,
                          t.bound_iters, t.cx_calls, t.cx_gains, t.search_iters, t.generations, t.cx_further_starts, t.lp_solves, t.lp_iters};
    std::copy(v, v + 16, out);
    return KAO_OK;
}
int kao_last_solve_profile(double out[8]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    const SolveProfile &p = g_last.profile;
    const double v[8] = {p.ms_search, p.ms_eval, p.search_launches, p.restarts, p.search_bytes_algo, p.delta_candidates, p.lds_bytes_search, p.blocks_search};
    std::copy(v, v + 8, out);
    return KAO_OK;
}
}  // extern "C"
