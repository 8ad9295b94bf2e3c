// kao_session.cpp -- sessions: the resident state of a batch of topics on one device (see kao_host.h).  Creating one is four steps:
// resolve the options, plan (pools, offsets, where each topic's assignment lives, launch groups, block maps: host work only), lay out
// the two device arenas, upload.  Then the K-search / K-eval step and the read-back; K-bound on a session is kao_session_bound.cpp.
// Everything that computes runs in the gfx950 kernels (kao_search.hip, kao_eval.hip).  There is deliberately no CPU evaluation or
// search path here: if the HIP device is missing every compute entry point fails with KAO_ERR_NO_DEVICE.
#include <cstring>

#include "kao_host.h"

namespace {

constexpr int kEvRing = 32;
constexpr const char *kChunkGaveUp = "K-search: a chunk gave up waiting for the chunk before it";

// Physical workgroup order: the dispatcher places workgroup b on XCD b % 8 (observed, used for L2
// affinity only), so the workgroups of one topic -- which read the same tables -- are dealt to one XCD.
template <typename Item>
std::vector<Item> xcd_order(const std::vector<Item> &items, const std::vector<int> &topic_of) {
    const size_t n = items.size();
    std::vector<std::vector<size_t>> q(8);
    for (size_t i = 0; i < n; ++i) q[(size_t)topic_of[i] % 8].push_back(i);
    std::vector<size_t> head(8, 0);
    std::vector<Item> out;
    out.reserve(n);
    for (size_t b = 0; b < n; ++b) {
        size_t x = b % 8;
        if (head[x] >= q[x].size()) {  // this XCD's queue ran dry: steal from the longest remaining one
            size_t bestx = 0, bestlen = 0;
            for (size_t y = 0; y < 8; ++y)
                if (q[y].size() - head[y] > bestlen) { bestlen = q[y].size() - head[y]; bestx = y; }
            x = bestx;
            out.push_back(items[q[x].back()]);
            q[x].pop_back();
            continue;
        }
        out.push_back(items[q[x][head[x]++]]);
    }
    return out;
}

int session_drain_events(kao_session *s) {
    for (int i = 0; i < s->ev_pending; ++i) {
        float a = 0, b = 0;
        HIP_TRY(hipEventSynchronize(s->ev[i * 3 + 2]));
        HIP_TRY(hipEventElapsedTime(&a, s->ev[i * 3 + 0], s->ev[i * 3 + 1]));
        HIP_TRY(hipEventElapsedTime(&b, s->ev[i * 3 + 1], s->ev[i * 3 + 2]));
        s->ms_search += a;
        s->ms_eval += b;
    }
    s->ev_pending = 0;
    return KAO_OK;
}

// The caller's options with every default filled in and every cap applied.  A pure function of its arguments: `n_cu` compute units,
// `device_bytes` of device memory in total (0: unknown).
int resolve_opts(const kao_topic *topics, int n_topics, const kao_opts *opts_in, int n_cu, uint64_t device_bytes, kao_opts &o) {
    o = opts_in ? *opts_in : kao_opts{};
    if (o.team < 0 || o.team > kTeamMax || o.schedule < 0 || o.schedule > 1) return fail(KAO_ERR_INVALID, "kao_opts: team must be 0..8, schedule 0 or 1");
    if (o.iters_per_launch <= 0) o.iters_per_launch = 512;
    if (o.obj_scale <= 0) o.obj_scale = 4;
    if (o.lam_min <= 0) o.lam_min = 1;
    if (o.lam_max <= 0) o.lam_max = 40;
    if (o.lam_max < o.lam_min) o.lam_max = o.lam_min;
    if (o.period_log2 < 0) o.period_log2 = 0;    // 0 = per topic, by size (auto_period_log2)
    if (o.period_log2 > 20) o.period_log2 = 20;
    if (o.time_limit_s <= 0) o.time_limit_s = 10.0;
    if (o.elite_period < 0) o.elite_period = 0;  // sessions: 0 = never (kao_solve picks its own default before creating the session)
    if (o.restarts <= 0) {  // automatic: one full round of resident wavefronts (8 per SIMD = 32 per CU) across all topics
        const int want = n_cu * 32;
        int r = want / n_topics;
        r = (r / kWaves) * kWaves;
        o.restarts = std::min(std::max(r, 8), 8192);
        // large topics need depth (iterations per second) more than breadth: at most 2^22 replica slots over all the
        // restarts of the largest topic, but never fewer than one restart per compute unit
        int64_t slots = 1;
        for (int t = 0; t < n_topics; ++t) slots = std::max<int64_t>(slots, (int64_t)topics[t].n_partitions * std::max(topics[t].rf, 1));
        // (round 4: four per compute unit where the topic lives in HBM -- a restart is then one wavefront waiting on dependent global
        //  loads, and 1024 of them take the time of 256: drifted 1000 x 30000 3.98 -> 4.43 ms per launch, profiles/r04_a_fill_probe.txt)
        const int floor_r = slots >= 32768 ? 4 * n_cu : n_cu;
        const int cap = (int)std::max<int64_t>(floor_r, (((int64_t)1 << 22) / slots) / kWaves * kWaves);
        o.restarts = std::min(o.restarts, cap);
        // a single topic whose WORKING assignment alone fits LDS (k_search_curg, ~4,900 .. 9,800 partitions): one wavefront per workgroup
        // and compute unit, so a count a little above the compute units (2^22 / slots = 276 at 5,000 partitions) would pay a whole second
        // round of workgroups for 20 restarts
        if (n_topics == 1 && o.restarts > n_cu && o.restarts <= n_cu + n_cu / 4 && o.team <= 1) {
            const kao_topic &t0 = topics[0];
            std::vector<int> rs((size_t)std::max(t0.n_racks, 1), 0);
            for (int b = 0; b < t0.n_brokers; ++b) if (t0.rack_of[b] < rs.size()) rs[t0.rack_of[b]]++;
            const int bx = *std::max_element(rs.begin(), rs.end()) * t0.n_racks, nw0 = (t0.rf > kRFP || t0.rf_cur > kRFP) ? 2 * kRFP : kRFP;
            const bool hbw = t0.broker_w || t0.broker_wl;
            if (search_lds_bytes(t0.n_partitions, bx, 1, false, true, nw0, hbw, t0.n_racks) > kLdsLimit &&
                search_lds_bytes(t0.n_partitions, bx, 1, false, true, nw0, hbw, t0.n_racks, 0, true) <= kLdsLimit)
                o.restarts = n_cu / kWaves * kWaves;
        }
    }
    if (o.restarts > (1 << 20) - 2) o.restarts = (1 << 20) - 2;  // id 0xFFFFF is reserved (kExternalRestart)
    // huge topics: bound the per-restart state in HBM (16 B of working words + the snapshot per partition):
    // at most 8 GB and at most a quarter of what the device has free right now (the constant assumed the 288 GB
    // device with nothing beside the session; multi-GPU replicas and capped rounds hold several sessions)
    uint64_t per_restart = 0;
    for (int t = 0; t < n_topics; ++t) per_restart += (uint64_t)topics[t].n_partitions * (32 + 2 * (uint64_t)std::max(topics[t].rf, 1));
    uint64_t budget = 8ull << 30;
    // keyed to the device's TOTAL memory, not to what happens to be free (same input, same seed, same answer whatever else
    // occupies the device; an allocation that does not fit fails loudly with KAO_ERR_NOMEM instead of changing the search)
    if (device_bytes > 0) budget = std::min<uint64_t>(budget, std::max<uint64_t>(device_bytes / 8, 256ull << 20));
    const uint64_t cap = budget / std::max<uint64_t>(per_restart, 1);
    if ((uint64_t)o.restarts > cap) o.restarts = (int)std::max<uint64_t>(cap / kWaves * kWaves, kWaves);
    return KAO_OK;
}

// What planning hands to the arena layout and the upload: the host images of the read-only pools, and the sizes of the mutable ones.
struct SessionPlan {
    std::vector<TopicDev> tds;
    std::vector<int2> smap;   // K-search workgroups: {topic, first restart}
    std::vector<int4> emap;   // K-eval workgroups: {topic, first candidate, n candidates, out base}
    std::vector<uint32_t> cur_pool, bw_pool, bwd_pool; std::vector<uint16_t> ext_pool, curd_pool, int_pool; std::vector<int32_t> rsz_pool;
    std::vector<uint8_t> rackof_pool;
    std::vector<int4> sched;  // chunked K-search: every chunking group's schedule, ticket -> {entry, chunk | chunks << 8, first iteration, iterations}
    uint64_t state_bytes = 0, best_u16 = 0, win_u16 = 0, dual_i32 = 0, price_i32 = 0, wide_slices = 0;
};
template <typename T>
uint32_t append(std::vector<T> &pool, const std::vector<T> &v) { pool.insert(pool.end(), v.begin(), v.end()); return (uint32_t)(pool.size() - v.size()); }

// One topic's share of every pool, its TopicDev offsets, and where its assignment lives (LDS / k_search_curg / HBM).
void plan_topic(kao_session &s, int t, bool curg_on, int n_cu, SessionPlan &pl) {
    const kao_opts &o = s.opts;
    const PreparedTopic &pt = s.pts[(size_t)t];
    TopicDev &d = s.pts[(size_t)t].d;
    d.n_restarts = o.restarts;
    d.period_log2 = o.period_log2 > 0 ? o.period_log2 : auto_period_log2(d.P, d.RF);
    d.restart_base = t * o.restarts;
    std::vector<uint32_t> &cur_pool = pl.cur_pool;
    while (cur_pool.size() % 4) cur_pool.push_back(kNoneW);   // every topic's words start 16-byte aligned
    d.cur_off = (uint32_t)cur_pool.size();
    for (size_t i = 0; i < (size_t)d.P * d.nw; ++i) cur_pool.push_back(replica_word(pt.cur_int[i], d.m));
    {   // the holes best insertion has to fill (slots below RF without a surviving replica): leader holes, then follower holes
        d.hole_off = (uint32_t)cur_pool.size();
        const size_t w0 = (size_t)d.cur_off;
        std::vector<uint32_t> lead, foll;
        for (int p = 0; p < d.P; ++p) {
            bool fh = false;
            for (int k = 1; k < d.RF; ++k) fh |= cur_pool[w0 + (size_t)p * d.nw + k] == kNoneW;
            if (cur_pool[w0 + (size_t)p * d.nw] == kNoneW) lead.push_back((uint32_t)p);
            if (fh) foll.push_back((uint32_t)p);
        }
        cur_pool.push_back((uint32_t)lead.size()); cur_pool.push_back((uint32_t)foll.size());
        append(cur_pool, lead);
        append(cur_pool, foll);
    }
    // both assignments in LDS when they fit (one wavefront per workgroup at least); else the working one alone, the current one read
    // from global memory / L2 (round 5: ~4,900 .. 9,800 partitions; KAO_CUR_GLOBAL=0: the HBM path as before); else everything in HBM
    const bool both_fit = search_lds_bytes(d.P, d.Bx, 1, false, true, d.nw, s.any_bw, d.R) <= kLdsLimit;
    // (one workgroup of ONE wavefront per restart and compute unit: with more restarts than compute units the workgroups run in rounds
    // and the HBM path, four wavefronts per workgroup, is the faster one -- 500 x 5000: 3.1 against 3.9 ms a launch at 256 restarts,
    // 12.4 against 4.2 at 1,024; teams (kao_opts.team) are a global-memory mode)
    const bool curg = !both_fit && curg_on && o.team <= 1 && o.restarts <= n_cu &&
                      search_lds_bytes(d.P, d.Bx, 1, false, true, d.nw, s.any_bw, d.R, 0, true) <= kLdsLimit;
    const bool global_a = !both_fit && !curg;
    s.topic_global[(size_t)t] = global_a;
    s.topic_curg[(size_t)t] = curg;
    d.ext_off = append(pl.ext_pool, pt.ext_of);
    d.rsz_off = append(pl.rsz_pool, pt.rack_size);
    d.state_off = pl.state_bytes;  // bytes: 8 per partition (packed, LDS path) or 16 (working words, global path)
    pl.state_bytes += align_up((uint64_t)o.restarts * d.P * d.nw * (global_a ? 4 : 2));
    d.best_off = pl.best_u16;
    pl.best_u16 += (uint64_t)o.restarts * d.P * d.RF;
    d.win_off = (uint32_t)pl.win_u16;
    pl.win_u16 += (uint64_t)d.P * d.RF;
    d.rackof_off = append(pl.rackof_pool, pt.rack_of);
    d.curd_off = append(pl.curd_pool, pt.cur_dense);
    if (d.has_bw) {
        d.bw_off = append(pl.bw_pool, pt.bw_int);
        d.bwd_off = append(pl.bwd_pool, pt.bw_dense);
        s.priced = true;   // broker weights live in the tables of the priced K-search instantiation
        s.any_bw = true;
    }
    d.int_off = append(pl.int_pool, pt.int_of);
    d.price_off = (uint32_t)pl.price_i32;
    pl.price_i32 += 2 * (uint64_t)d.B + kRackTab;
    pl.dual_i32 = (pl.dual_i32 + 1) & ~(uint64_t)1;  // the level-control words are 64-bit
    d.dual_off = (uint32_t)pl.dual_i32;
    pl.dual_i32 += 6 * (uint64_t)d.B + 3 * kRackTab + 8;
    d.cnt_off = (uint32_t)pl.dual_i32;             // counters of the sliced K-bound live in the same pool (zeroed with it)
    pl.dual_i32 += 3 * (2 * (uint64_t)d.B + kRackTab) + 4 * (uint64_t)d.B + 2 * kRackTab;   // x 3 + shadow area: k_bound_multi
    pl.wide_slices += (uint64_t)(d.P + 63) / 64;
    // algorithmic bytes: full evaluation = 2*RF*P + 2*rf_cur*P + B per candidate
    s.eval_bytes_per_launch += (uint64_t)o.restarts * (uint64_t)(2 * d.RF * d.P + 2 * d.rf_cur * d.P + d.B);
}

// Launch groups: topics sorted by single-wave LDS need, a new group whenever the need doubles (<= 8 groups); per group the kernel
// shapes and both block maps.
int plan_groups(kao_session &s, int n_cu, SessionPlan &pl) {
    const kao_opts &o = s.opts;
    const bool rft_on = env_int("KAO_SEARCH_RFT", 1) != 0;   // (read per session: a test hook; 0 = the generic K-search kernel throughout)
    s.small_on = env_int("KAO_SEARCH_SMALL", 1) != 0;        // (the same kind of hook; 0 = the RF-3 kernel always with the general cost arithmetic)
    std::vector<int> order((size_t)s.n_topics);
    for (int t = 0; t < s.n_topics; ++t) order[(size_t)t] = t;
    auto need1 = [&](int t) {  // topics kept in global memory sort last (their LDS need is tiny but they form their own groups)
        const TopicDev &d = s.pts[(size_t)t].d;
        const bool ga = s.topic_global[(size_t)t] != 0;
        const bool cg = s.topic_curg[(size_t)t] != 0;
        return (ga ? ((size_t)1 << 40) : 0) + (cg ? ((size_t)1 << 39) : 0) + (d.nw > kRFP ? ((size_t)1 << 41) : 0) + search_lds_bytes(d.P, d.Bx, 1, ga, true, d.nw, s.any_bw, d.R, 0, cg);
    };
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return need1(x) < need1(y); });
    std::vector<std::vector<int>> members;
    size_t group_base = 0;
    // K-search / K-eval are instantiated per (assignment words in HBM or LDS, words per partition): a launch group must be
    // homogeneous in both, whatever the LDS sizes say -- so a change of either ALWAYS starts a group; the
    // "at most 8 groups" cap only limits the splits by LDS footprint
    auto kind = [&](int t) { return (s.topic_global[(size_t)t] ? 1 : 0) | (s.pts[(size_t)t].d.nw > kRFP ? 2 : 0) | (s.topic_curg[(size_t)t] ? 4 : 0); };
    int lds_groups = 0, group_kind = -1;
    for (int t : order) {
        const bool new_kind = members.empty() || kind(t) != group_kind;
        if (new_kind || (need1(t) > 2 * group_base && lds_groups < 8)) {
            members.emplace_back(); group_base = need1(t); group_kind = kind(t);
            if (new_kind) lds_groups = 1; else ++lds_groups;
        }
        members.back().push_back(t);
    }
    for (const std::vector<int> &mem : members) {
        kao_session::LaunchGroup g;
        // candidates (one best snapshot per restart) per K-eval workgroup: 32 when the group fills the device; fewer when it does
        // not (a 30,000-partition topic has 256 restarts: at 32 per workgroup that was EIGHT workgroups, 2.9 ms per step --
        // a third of the step); few large candidates get one workgroup each, its wavefronts cooperating (k_eval<NE, true>)
        int64_t n_cand = 0;
        for (int t : mem) n_cand += s.pts[(size_t)t].d.n_restarts;
        const int64_t fill = 4 * (int64_t)std::max(n_cu, 1);
        int cpb = 32;
        if (n_cand < fill * 32) cpb = (int)std::min<int64_t>(32, std::max<int64_t>(kWaves, ((n_cand + fill - 1) / fill + kWaves - 1) / kWaves * kWaves));
        for (int t : mem) {
            const TopicDev &d = s.pts[(size_t)t].d;
            g.rf_uniform = g.rf_uniform < 0 ? d.RF : (g.rf_uniform == d.RF ? d.RF : 0);
            for (const int w : {d.w00, d.w01, d.w10, d.w11}) g.w_abs_max = std::max(g.w_abs_max, w < 0 ? (w == INT32_MIN ? INT32_MAX : -w) : w);
            g.band_tabs = g.band_tabs && search_band_tabs(d.rep_lo, d.rep_hi, d.lead_lo, d.lead_hi);
            g.rf3 = g.rf3 && d.RF == 3 && d.rf_cur <= 3;   // (RF 3 with four current replicas: word 3 of CUR is a real replica)
            g.maxP = std::max(g.maxP, d.P); g.maxBx = std::max(g.maxBx, d.Bx); g.maxB = std::max(g.maxB, d.B); g.maxR = std::max(g.maxR, d.R); g.wide = g.wide || (int64_t)d.P * d.RF >= 512;
        }
        g.rf3 = g.rf3 && rft_on;
        g.global_a = s.topic_global[(size_t)mem[0]] != 0;
        g.cur_global = s.topic_curg[(size_t)mem[0]] != 0;
        g.nw = s.pts[(size_t)mem[0]].d.nw;
        g.eval_coop = n_cand <= fill && g.maxP >= 1024;
        if (g.eval_coop) cpb = 1;
        // Topics that live in global memory: a restart is latency-bound (dependent loads of 16-byte assignment words), so ONE
        // wavefront per restart leaves the restart shallow.  Round 4 tried a TEAM of wavefronts per restart (k_team): W proposals
        // per iteration against the same state, the disjoint ones applied.  Measured (gpurun_out/r04_c2_*): same iterations per
        // second per restart at team 2 / 4, fewer at 8, and the 3-s incumbents of 1000 x 30000 / 1000 x 100000 within noise of
        // one wavefront per restart -- so teams are opt-in (kao_opts.team = n), the default is k_search.
        if (g.global_a) {
            const int tmax = g.nw > kRFP ? kTeamMax / 2 : kTeamMax;   // (8 replica words per partition: 256 threads keep the kernel out of scratch)
            const int want = o.team == 0 ? 1 : o.team;
            g.team = want <= 1 ? 0 : std::min(want, tmax);
            if (g.team > 0) g.waves = 1;   // the block map holds one workgroup per restart
        }
        auto search_lds = [&] { return search_lds_bytes(g.maxP, g.maxBx, g.waves, g.global_a, true, g.nw, s.any_bw, g.maxR, g.team, g.cur_global); };
        while (g.waves > 1 && search_lds() > kLdsLimit) g.waves /= 2;
        g.cur_in_lds = eval_lds_bytes(g.maxP, g.maxB, true, g.nw) <= kLdsLimit;
        if (search_lds() > kLdsLimit || eval_lds_bytes(g.maxP, g.maxB, g.cur_in_lds, g.nw) > kLdsLimit)
            return fail(KAO_ERR_UNSUPPORTED, "broker tables exceed 160 KiB of LDS (about 30,000 padded brokers)");
        std::vector<int2> gs; std::vector<int> gs_topic;
        std::vector<int4> ge; std::vector<int> ge_topic;
        for (int t : mem) {
            const TopicDev &d = s.pts[(size_t)t].d;
            for (int r = 0; r < d.n_restarts; r += g.waves) { gs.push_back(make_int2(t, r)); gs_topic.push_back(t); }
            for (int r = 0; r < d.n_restarts; r += cpb) {
                ge.push_back(make_int4(t, r, std::min(cpb, d.n_restarts - r), d.restart_base + r));
                ge_topic.push_back(t);
            }
        }
        gs = xcd_order(gs, gs_topic);
        ge = xcd_order(ge, ge_topic);
        g.smap_off = (int)pl.smap.size(); g.smap_n = (int)gs.size();
        g.emap_off = (int)pl.emap.size(); g.emap_n = (int)ge.size();
        pl.smap.insert(pl.smap.end(), gs.begin(), gs.end());
        pl.emap.insert(pl.emap.end(), ge.begin(), ge.end());
        s.groups.push_back(g);
    }
    s.blocks_search = (int)pl.smap.size();
    s.blocks_eval = (int)pl.emap.size();
    return KAO_OK;
}

// Everything the search will do, decided on the host from s.opts (resolved) and the topics: the prepared topics with their pool
// offsets, where each topic's assignment lives, what K-bound can cover, the launch groups and block maps.  Touches no device.
int plan_session(kao_session &s, const kao_topic *topics, int n_cu, SessionPlan &pl) {
    const int n_topics = s.n_topics;
    s.pts.resize((size_t)n_topics);
    s.topics.assign(topics, topics + n_topics);
    s.ub.resize((size_t)n_topics);
    s.topic_global.assign((size_t)n_topics, 0);
    s.topic_curg.assign((size_t)n_topics, 0);
    for (int t = 0; t < n_topics; ++t) s.any_bw |= topics[t].broker_w || topics[t].broker_wl;
    const bool curg_on = env_int("KAO_CUR_GLOBAL", 1) != 0;   // (read per session: a test hook)
    for (int t = 0; t < n_topics; ++t) {
        const uint64_t seed = s.opts.seed ^ ((uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull);
        const int rc = prepare(&topics[t], seed, s.pts[(size_t)t]);
        if (rc) return rc;
        s.ub[(size_t)t] = upper_bound_w(&topics[t]);
        s.topic_infeasible.push_back(infeasible_reason(&topics[t]).empty() ? 0 : 1);
        plan_topic(s, t, curg_on, n_cu, pl);
        s.dual_ok.push_back(dual_supported(&topics[t], s.any_bw) ? 1 : 0);
    }
    s.dual_flags.assign((size_t)n_topics, 0);
    s.dual_iters.assign((size_t)n_topics, 0);
    for (int t = 0; t < n_topics; ++t) if (!s.dual_ok[(size_t)t]) s.dual_flags[(size_t)t] = 8;
    s.total_restarts = n_topics * s.opts.restarts;
    const int rc = plan_groups(s, n_cu, pl);
    for (const PreparedTopic &pt : s.pts) pl.tds.push_back(pt.d);
    return rc;
}

// Does the group's K-search run its small-cost form?  (The options it depends on are the session's: the same answer at every step.)
bool group_small(const kao_session &s, const kao_session::LaunchGroup &g) {
    const bool rf3_runs = g.rf3 && search_rf3_eligible(g.global_a, g.cur_global, s.priced, g.nw, g.team);
    return rf3_runs && s.small_on && g.band_tabs && search_small_cost(s.opts.lam_min, s.opts.lam_max, s.opts.obj_scale, g.w_abs_max, s.priced);
}

}  // namespace

namespace kao {
// The schedule of a chunked launch.  Two shapes, both chunk-major over the entries they chunk, so that an entry's chunks are as many
// tickets apart as there are chunked entries and the tickets dispatched last -- the ones the device empties on -- are last chunks,
// pieces of 1 / C of a launch:
//   forced (KAO_SEARCH_CHUNKS=N): every entry in N chunks, ticket c * entries + e = chunk c of entry e;
//   automatic (only from kChunkMinRounds resident rounds of entries on: with fewer, most of the batch would be tail and pay the
//     hand-off, the uniform shape that measured worse; kao_solve's default batch of 1.3 rounds stays in one piece): only a tail is chunked -- the last K entries of the block map, K = kChunkTailPct of the resident workgroups -- and
//     everything in front of it stays one piece: tickets 0 .. entries - K - 1 are whole entries, then chunk c of tail entry e is
//     ticket (entries - K) + c * K + (e - (entries - K)).  A hand-off costs about 1.6 % of a 128-iteration chunk (docs/notes_r16.md):
//     the tail pays it on K / entries of the work only.  K of one resident round is the default (tails of 100 and 150 % compared on one build, 200 / 300 % on another:
//     docs/notes_r16.md): the chunk before was taken a whole round of tickets earlier and has all but finished when its successor
//     starts to wait.
// The iterations are split evenly, the first iters % C chunks one longer.
int search_chunk_plan(int entries, int resident, int iters, int forced, int32_t *out) {
    if (entries < 1) return 0;
    iters = std::max(iters, 0);
    int C = 1, K = entries;
    if (forced >= 2) C = std::min(forced, kChunkMax);
    else if (forced == 0 && entries >= kChunkMinRounds * (int64_t)std::max(resident, 1)) {
        C = kChunkAuto;
        while (C > 1 && iters / C < kChunkMinIters) C /= 2;
        K = (int)std::min<int64_t>(entries, std::max<int64_t>(1, (int64_t)std::max(resident, 1) * kChunkTailPct / 100));
    }
    C = std::max(1, std::min(C, iters));   // no empty chunk: fewer chunks when there are fewer iterations
    if (C == 1) K = entries;
    const int whole = entries - K;          // entries in front of the tail: one piece each
    if (out) {
        for (int e = 0; e < whole; ++e) { int32_t *o = out + 4 * (size_t)e; o[0] = e; o[1] = 0; o[2] = 0; o[3] = iters; }
        for (int c = 0; c < C; ++c) {
            const int first = c * (iters / C) + std::min(c, iters % C), n = iters / C + (c < iters % C ? 1 : 0);
            for (int e = 0; e < K; ++e) {
                int32_t *o = out + 4 * ((size_t)whole + (size_t)c * K + e);
                o[0] = whole + e; o[1] = c; o[2] = first; o[3] = n;
            }
        }
    }
    return whole + C * K;
}
}  // namespace kao

extern "C" int kao_search_chunk_plan(int32_t entries, int32_t resident, int32_t iters, int32_t forced, int32_t *out, int32_t cap) {
    if (entries < 1 || resident < 0 || iters < 0 || forced < 0) return fail(KAO_ERR_INVALID, "kao_search_chunk_plan: bad argument");
    const int n = kao::search_chunk_plan(entries, resident, iters, forced, nullptr);
    if (out && cap >= n) kao::search_chunk_plan(entries, resident, iters, forced, out);
    return n;
}

namespace {

// K-search as ticketed chunks: per eligible launch group the schedule search_chunk_plan gives for its entries, the workgroups the
// device holds of its kernel (the runtime's occupancy query x compute units) and the session's iterations per launch.  A group whose
// plan has one ticket per entry launches exactly as before.
void plan_chunks(kao_session &s, int n_cu, SessionPlan &pl) {
    s.chunks_forced = (int)std::min<int64_t>(std::max<int64_t>(env_int("KAO_SEARCH_CHUNKS", 0), 0), kChunkMax);   // (read per session: a test hook)
    if (s.chunks_forced == 1) return;
    for (kao_session::LaunchGroup &g : s.groups) {
        if (!search_chunk_eligible(g.global_a, g.cur_global, g.team)) continue;
        // The automatic rule chunks only what has been measured to win: the small-cost RF-3 kernel of topics below 512 replica slots
        // (the benchmark's shape, +4.6 %, docs/notes_r16.md).  The chunked kernels of the other instantiations -- wide, general cost,
        // generic RF, priced -- carry more scratch than the kernels they would replace and have not been timed on an oversubscribed
        // batch: they run only when KAO_SEARCH_CHUNKS=N forces them.
        if (s.chunks_forced == 0 && !(group_small(s, g) && !g.wide)) continue;
        // (a compute unit holds at least one workgroup: a group of no more entries than compute units is one resident round whatever
        //  the occupancy, and a launch too short for two chunks of kChunkMinIters never chunks -- no query for kao_solve's sessions)
        if (s.chunks_forced == 0 && (g.smap_n <= std::max(n_cu, 1) || s.opts.iters_per_launch < 2 * kChunkMinIters)) continue;
        const size_t lds = search_lds_bytes(g.maxP, g.maxBx, g.waves, false, s.priced, g.nw, s.any_bw, g.maxR, 0, false);
        const int per_cu = search_resident_blocks(g.waves, s.priced, g.nw, g.wide, g.rf3 ? 3 : 0, group_small(s, g), lds);
        const int resident = per_cu > 0 ? per_cu * std::max(n_cu, 1) : INT32_MAX;   // (query failed: the automatic rule never chunks)
        const int iters = s.opts.iters_per_launch;
        const int tickets = search_chunk_plan(g.smap_n, resident, iters, s.chunks_forced, nullptr);
        if (tickets <= g.smap_n) continue;
        std::vector<int32_t> plan((size_t)tickets * 4);
        search_chunk_plan(g.smap_n, resident, iters, s.chunks_forced, plan.data());
        g.chunk_tickets = tickets;
        g.chunk_n = 1;
        for (int t = 0; t < tickets; ++t) g.chunk_n = std::max(g.chunk_n, plan[(size_t)t * 4 + 1] + 1);
        g.chunk_iters = iters;
        g.chunk_priced = s.priced;
        g.sched_off = (int)pl.sched.size();
        std::vector<int> per_entry((size_t)g.smap_n, 0);
        for (int t = 0; t < tickets; ++t) per_entry[(size_t)plan[(size_t)t * 4]]++;
        for (int t = 0; t < tickets; ++t) {
            const int32_t *r = &plan[(size_t)t * 4];
            pl.sched.push_back(make_int4(r[0], r[1] | (per_entry[(size_t)r[0]] << 8), r[2], r[3]));
        }
        s.can_chunk = true;
    }
}

// The sections of one device arena in order, each starting on a 256-byte boundary.  A section is added once, with the session's
// pointer to it, its size and (read-only arena) the host image to upload: offsets, the total, the staging copy and the device
// pointers all come from this one list.
struct ArenaLayout {
    struct Sec { void *slot; size_t off, bytes; const void *src; };
    std::vector<Sec> secs;
    size_t total = 0;
    template <typename T>
    void add(T *&dev_ptr, size_t bytes, const void *src = nullptr) {
        secs.push_back({&dev_ptr, total, bytes, src});
        total += align_up(bytes);
    }
    template <typename T, typename V>
    void add(T *&dev_ptr, const std::vector<V> &image) { add(dev_ptr, image.size() * sizeof(V), image.data()); }
    void stage(unsigned char *host) const {
        for (const Sec &sec : secs) if (sec.bytes && sec.src) std::memcpy(host + sec.off, sec.src, sec.bytes);
    }
    void bind(void *base) const {   // every registered pointer = base + its section's offset
        for (const Sec &sec : secs) { unsigned char *p = static_cast<unsigned char *>(base) + sec.off; std::memcpy(sec.slot, &p, sizeof p); }
    }
};

// read-only arena: the instance tables, staged on the host and uploaded with ONE H2D copy
ArenaLayout layout_ro(kao_session &s, const SessionPlan &pl) {
    ArenaLayout a;
    a.add(s.d_topics, pl.tds);
    a.add(s.d_smap, pl.smap);
    a.add(s.d_emap, pl.emap);
    a.add(s.d_cur, pl.cur_pool);
    a.add(s.d_ext, pl.ext_pool);
    a.add(s.d_rsz, pl.rsz_pool);
    a.add(s.d_rackof, pl.rackof_pool);
    a.add(s.d_curd, pl.curd_pool);
    a.add(s.d_int, pl.int_pool);
    a.add(s.d_bw, pl.bw_pool);
    a.add(s.d_bwd, pl.bwd_pool);
    if (s.can_chunk) a.add(s.d_sched, pl.sched);
    return a;
}

// mutable arena: restart states, snapshots, results, the read-back block, K-bound's pool and staging, the two price halves
ArenaLayout layout_rw(kao_session &s, const SessionPlan &pl) {
    const size_t n_topics = (size_t)s.n_topics, n_restarts = (size_t)s.total_restarts;
    // read-back block (one D2H): [keys u64[T]] [drift i32 (16 B)] [win_viol i32[8T]] [win_assign u16[sum P*RF]]
    s.rb_viol_off = align_up(n_topics * 8 + 16, 16);
    s.rb_assign_off = s.rb_viol_off + n_topics * 32;
    s.readback_bytes = s.rb_assign_off + pl.win_u16 * 2;
    // K-bound's pool: behind the per-topic blocks, control blocks (8 x int64 per topic) and the workgroup map of the sliced drivers
    uint64_t dual_i32 = (pl.dual_i32 + 1) & ~(uint64_t)1;
    s.wide_ctl_i32 = dual_i32; dual_i32 += 32 * (uint64_t)n_topics;
    s.wide_map_i32 = dual_i32; dual_i32 += 2 * pl.wide_slices;
    s.dual_bytes = align_up(dual_i32 * 4);
    s.dual_rb_bytes = n_topics * 24;
    s.price_half_i32 = align_up(pl.price_i32 * 4) / 4;
    s.best_bytes = pl.best_u16 * 2 ? pl.best_u16 * 2 : 2;
    ArenaLayout a;
    a.add(s.d_state, pl.state_bytes);
    a.add(s.d_best, pl.best_u16 * 2);
    a.add(s.d_info, n_restarts * 16);
    a.add(s.d_obj, n_restarts * 4);
    a.add(s.d_viol, n_restarts * 32);
    a.add(s.d_readback, s.readback_bytes);
    a.add(s.d_dual, s.dual_bytes);
    a.add(s.d_dual_target, n_topics * 8);
    a.add(s.d_dual_ids, n_topics * 4);
    a.add(s.d_dual_rb, s.dual_rb_bytes);
    a.add(s.d_price, 2 * s.price_half_i32 * 4);
    a.add(s.d_keys_glob, n_topics * 8);
    if (s.can_chunk) {   // (sessions that never chunk carry none of this: the generator words are 256 B per restart)
        a.add(s.d_chunk_ctl, 256);
        a.add(s.d_chunk_progress, (size_t)s.blocks_search * 4);
        a.add(s.d_chunk_rng, n_restarts * 256);
    }
    return a;
}

}  // namespace

extern "C" {

void kao_session_destroy(kao_session *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->stream_bound) (void)hipStreamSynchronize(s->stream_bound);
    if (s->ev_bound0) (void)hipEventDestroy(s->ev_bound0);
    if (s->ev_bound1) (void)hipEventDestroy(s->ev_bound1);
    if (s->ev_search) (void)hipEventDestroy(s->ev_search);
    if (s->stream_bound) (void)hipStreamDestroy(s->stream_bound);
    if (s->h_chunk_err) (void)hipHostFree(s->h_chunk_err);
    arena_put(s->arena_ro, s->arena_ro_bytes, s->device);
    arena_put(s->arena_rw, s->arena_rw_bytes, s->device);
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    stream_put(s->stream, s->device);
    delete s;
}

int kao_session_create(const kao_topic *topics, int32_t n_topics, const kao_opts *opts_in, kao_session **out) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    *out = nullptr;
    if (!topics || n_topics < 1) return fail(KAO_ERR_INVALID, "no topics");
    int rc = require_init();
    if (rc) return rc;
    SessionPtr s(new kao_session());
    s->device = cur_device();
    s->n_topics = n_topics;
    const int n_cu = num_cu(s->device);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = 0;   // unknown: resolve_opts budgets for 8 GB
    if ((rc = resolve_opts(topics, n_topics, opts_in, n_cu, total_b, s->opts))) return rc;
    SessionPlan pl;
    if ((rc = plan_session(*s, topics, n_cu, pl))) return rc;
    plan_chunks(*s, n_cu, pl);

    const ArenaLayout ro = layout_ro(*s, pl), rw = layout_rw(*s, pl);
    if ((rc = arena_get(ro.total, &s->arena_ro, &s->arena_ro_bytes))) return rc;
    if ((rc = arena_get(rw.total, &s->arena_rw, &s->arena_rw_bytes))) return rc;
    ro.bind(s->arena_ro);
    rw.bind(s->arena_rw);
    s->d_keys = reinterpret_cast<unsigned long long *>(s->d_readback);
    s->d_drift = reinterpret_cast<int32_t *>(s->d_readback + (size_t)n_topics * 8);
    s->d_win_viol = reinterpret_cast<int32_t *>(s->d_readback + s->rb_viol_off);
    s->d_win_assign = reinterpret_cast<uint16_t *>(s->d_readback + s->rb_assign_off);
    s->h_readback.assign(s->readback_bytes, 0);
    std::vector<unsigned char> stage(ro.total);
    ro.stage(stage.data());

    if ((rc = stream_get(&s->stream))) return rc;
    // restart states / info / obj / viol are fully written by launch 0 (init) and the first K-eval; only the
    // snapshots ("no snapshot" = all KAO_NONE), the keys (all ones) and the drift counter need initial values
    const size_t price_b = 2 * s->price_half_i32 * 4;
    hipError_t e1 = hipMemcpyAsync(s->arena_ro, stage.data(), ro.total, hipMemcpyHostToDevice, s->stream);
    hipError_t e2 = hipMemsetAsync(s->d_best, 0xFF, s->best_bytes, s->stream);
    hipError_t e3 = hipMemsetAsync(s->d_readback, 0xFF, (size_t)n_topics * 8, s->stream);
    hipError_t e4 = hipMemsetAsync(s->d_drift, 0, 16, s->stream);
    if (e4 == hipSuccess) e4 = hipMemsetAsync(s->d_price, 0, price_b ? price_b : 4, s->stream);  // no prices yet
    if (s->can_chunk && e4 == hipSuccess) {   // (a failure is reported below, behind the synchronisation, with the others)
        e4 = hipHostMalloc(reinterpret_cast<void **>(&s->h_chunk_err), 16);
        if (e4 == hipSuccess) *s->h_chunk_err = 0; else s->h_chunk_err = nullptr;
    }
    if (s->can_chunk && e4 == hipSuccess) {   // ticket counter and progress words: zero once, never again (arenas are reused)
        e4 = hipMemsetAsync(s->d_chunk_ctl, 0, 256, s->stream);
        if (e4 == hipSuccess) e4 = hipMemsetAsync(s->d_chunk_progress, 0, (size_t)s->blocks_search * 4, s->stream);
    }
    hipError_t e5 = hipStreamSynchronize(s->stream);  // `stage` is pageable host memory and goes out of scope
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess) return fail(KAO_ERR_HIP, "session upload failed");
    if (s->opts.profile) {
        s->ev.resize(kEvRing * 3);
        for (auto &e : s->ev) if (hipEventCreate(&e) != hipSuccess) return fail(KAO_ERR_HIP, "hipEventCreate");
    }
    *out = s.release();
    return KAO_OK;
}

int kao_session_step(kao_session *s) {
    if (!s) return fail(KAO_ERR_INVALID, "null session");
    HIP_TRY(hipSetDevice(s->device));
    const bool prof = s->opts.profile != 0;
    if (prof && s->ev_pending == kEvRing) {
        int rc = session_drain_events(s);
        if (rc) return rc;
    }
    SearchPools sp{};
    sp.topics = s->d_topics; sp.block_map = s->d_smap; sp.cur_pool = s->d_cur; sp.ext_pool = s->d_ext; sp.rsz_pool = s->d_rsz;
    sp.state_pool = s->d_state; sp.best_pool = s->d_best; sp.restart_info = s->d_info; sp.drift = s->d_drift;
    SearchParams prm{};
    prm.obj_scale = s->opts.obj_scale; prm.lam_min = s->opts.lam_min; prm.lam_max = s->opts.lam_max;
    prm.launch = s->launch; prm.iters = (uint32_t)s->opts.iters_per_launch; prm.init = (s->launch == 0 || s->reinit) ? 1 : 0;
    prm.gen = s->gen;
    s->reinit = false;
    const int eper = s->opts.elite_period;
    prm.bw = s->any_bw ? 1 : 0;
    prm.scan2_max = kScanTwoSlots;
    prm.elite = (eper > 0 && s->launch > 0 && s->launch % (uint32_t)eper == 0) ? 1 : 0;
    sp.price_pool = s->d_price + (size_t)s->price_read * s->price_half_i32;
    sp.int_pool = s->d_int; sp.elite_assign = s->d_win_assign; sp.elite_key = s->d_keys; sp.bw_pool = s->d_bw;
    EvalPools ep{};
    ep.topics = s->d_topics; ep.rackof_pool = s->d_rackof; ep.curd_pool = s->d_curd;
    ep.cand = s->d_best; ep.objective = s->d_obj; ep.violations = s->d_viol; ep.best_key = s->d_keys; ep.bwd_pool = s->d_bwd;
    hipEvent_t *e = prof ? &s->ev[(size_t)s->ev_pending * 3] : nullptr;
    if (prof) HIP_TRY(hipEventRecord(e[0], s->stream));
    for (const kao_session::LaunchGroup &g : s->groups) {
        sp.block_map = s->d_smap + g.smap_off;
        prm.maxP = g.maxP; prm.maxBx = g.maxBx; prm.maxR = g.maxR; prm.wide = g.wide ? 1 : 0; prm.cur_global = g.cur_global ? 1 : 0;
        SearchParams gp = prm;
        if (gp.init && g.global_a) {   // topics in global memory: the holes are filled by a workgroup per restart (K-init), not by one wavefront
            const int init_waves = (int)env_int("KAO_INIT_WAVES", -1);   // measurement hook: wavefronts per restart (unset: automatic); 0 = the one-wavefront fill inside k_search
            if (init_waves != 0 && launch_init(sp, gp, g.smap_n, g.team > 0 ? 1 : g.waves, s->priced, g.nw, std::max(init_waves, 0), s->stream)) gp.init = 2;
            HIP_TRY(hipGetLastError());
        }
        const int rft = g.rf3 ? 3 : 0;
        const bool rf3_runs = rft && search_rf3_eligible(g.global_a, g.cur_global, s->priced, g.nw, g.team);
        const bool small = group_small(*s, g);
        int n_blocks = g.smap_n;
        // (the schedule splits the iterations it was planned for, with the kernel it was planned for: a step with another count --
        //  kao_solve's short first launch -- or with prices switched on since runs in one piece)
        if (g.chunk_tickets && (int)gp.iters == g.chunk_iters && s->priced == g.chunk_priced) {   // one workgroup per ticket; the progress words of this group's entries carry this launch's serial
            gp.chunks = g.chunk_n; gp.serial = ++s->chunk_serial;
            sp.chunk_ticket = s->d_chunk_ctl; sp.chunk_progress = s->d_chunk_progress + g.smap_off; sp.chunk_rng = s->d_chunk_rng;
            sp.chunk_sched = s->d_sched + g.sched_off;
            n_blocks = g.chunk_tickets;
            s->search_chunked_launches++;
        }
        launch_search(sp, gp, n_blocks, g.waves, g.global_a, s->priced, g.nw, s->stream, g.team, rft, small);
        if (rf3_runs) s->search_rf3_launches++;
        if (small) s->search_small_launches++;
        HIP_TRY(hipGetLastError());
    }
    if (prof) HIP_TRY(hipEventRecord(e[1], s->stream));
    for (const kao_session::LaunchGroup &g : s->groups) {
        ep.block_map = s->d_emap + g.emap_off;
        ep.maxP = g.maxP; ep.maxB = g.maxB; ep.cur_in_lds = g.cur_in_lds ? 1 : 0; ep.coop = g.eval_coop ? 1 : 0; ep.rf_uniform = std::max(g.rf_uniform, 0);
        launch_eval(ep, g.emap_n, g.nw, s->stream);
        HIP_TRY(hipGetLastError());
    }
    if (prof) { HIP_TRY(hipEventRecord(e[2], s->stream)); s->ev_pending++; }
    if (eper > 0 && (s->launch + 1) % (uint32_t)eper == 0) {  // the next launch is an elite launch: stage every topic's best assignment
        launch_gather(s->d_topics, s->n_topics, s->d_keys, s->d_best, s->d_viol, s->d_win_assign, s->d_win_viol, s->stream);
        HIP_TRY(hipGetLastError());
    }
    for (const PreparedTopic &pt : s->pts) {
        const uint64_t n = neighbours_in_range(prm.launch * prm.iters, prm.iters, pt.d.RF, pt.d.B, pt.d.P, prm.scan2_max) * (uint64_t)pt.d.n_restarts;
        s->delta_total += n;
        s->search_bytes_total += n * (uint64_t)(8 * pt.d.RF + 10);
    }
    s->launch++;
    return KAO_OK;
}

// A new generation of the population: the next step re-initialises every restart from the current assignment (best
// insertion, tie-break hash salted with the generation number), the snapshots and packed best keys of the old generation are
// dropped -- the caller has read what it wants to keep (kao_solve keeps the incumbent on the host).  K-bound state, prices
// and the launch / iteration counters carry on.
int kao_session_new_generation(kao_session *s) {
    if (!s) return fail(KAO_ERR_INVALID, "null session");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->d_best, 0xFF, s->best_bytes, s->stream));
    HIP_TRY(hipMemsetAsync(s->d_readback, 0xFF, (size_t)s->n_topics * 8, s->stream));   // packed best keys: none
    s->gen++;
    s->reinit = true;
    return KAO_OK;
}

int kao_session_sync(kao_session *s) {
    if (!s) return fail(KAO_ERR_INVALID, "null session");
    HIP_TRY(hipSetDevice(s->device));
    // (chunking sessions: the error word rides in front of the synchronisation, four bytes into pinned memory)
    if (s->h_chunk_err) HIP_TRY(hipMemcpyAsync(s->h_chunk_err, s->d_drift + 1, 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->h_chunk_err && *s->h_chunk_err) return fail(KAO_ERR_HIP, kChunkGaveUp);
    if (s->opts.profile) return session_drain_events(s);
    return KAO_OK;
}

int kao_session_best_keys(kao_session *s, uint64_t *keys) {
    if (!s || !keys) return fail(KAO_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    if (s->h_chunk_err) {   // chunking sessions: still ONE copy -- the drift block stands behind the keys in the read-back block
        const size_t nk = (size_t)s->n_topics * 8;
        HIP_TRY(hipMemcpyAsync(s->h_readback.data(), s->d_keys, nk + 8, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        std::memcpy(keys, s->h_readback.data(), nk);
        std::memcpy(s->h_chunk_err, s->h_readback.data() + nk + 4, 4);
        if (*s->h_chunk_err) return fail(KAO_ERR_HIP, kChunkGaveUp);
        return KAO_OK;
    }
    HIP_TRY(hipMemcpyAsync(keys, s->d_keys, (size_t)s->n_topics * 8, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return KAO_OK;
}

int kao_session_device_keys(kao_session *s, void **d_keys) {
    if (!s || !d_keys) return fail(KAO_ERR_INVALID, "null argument");
    *d_keys = s->d_keys;
    return KAO_OK;
}

int kao_session_best(kao_session *s, kao_result *results) {
    if (!s || !results) return fail(KAO_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->device));
    launch_gather(s->d_topics, s->n_topics, s->d_keys, s->d_best, s->d_viol, s->d_win_assign, s->d_win_viol, s->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->h_readback.data(), s->d_readback, s->readback_bytes, hipMemcpyDeviceToHost, s->stream));
    int rc = kao_session_sync(s);
    if (rc) return rc;
    const uint64_t *keys = reinterpret_cast<const uint64_t *>(s->h_readback.data());
    const int32_t *wv = reinterpret_cast<const int32_t *>(s->h_readback.data() + s->rb_viol_off);
    const uint16_t *wa = reinterpret_cast<const uint16_t *>(s->h_readback.data() + s->rb_assign_off);
    for (int t = 0; t < s->n_topics; ++t) {
        const TopicDev &d = s->pts[(size_t)t].d;
        kao_result &r = results[t];
        r.upper_bound = s->ub[(size_t)t];
        const uint64_t key = keys[t];
        if (key == ~0ull) {  // no step has run yet
            r.status = s->topic_infeasible[(size_t)t] ? KAO_STATUS_INFEASIBLE_PROVEN : KAO_STATUS_NO_FEASIBLE; r.best_restart = -1; r.objective = -1;
            std::memset(r.violations, 0, sizeof r.violations);
            continue;
        }
        r.best_restart = (key & 0xFFFFF) == kExternalRestart ? -1 : (int)(key & 0xFFFFF);  // -1: adopted from another GPU
        r.objective = (int64_t)kObjCap - (int64_t)((key >> 20) & 0xFFFFFF);
        std::memcpy(r.violations, wv + (size_t)t * 8, 32);
        if (r.assignment) std::memcpy(r.assignment, wa + d.win_off, (size_t)d.P * d.RF * 2);
        if (r.violations[0] != 0) { r.status = s->topic_infeasible[(size_t)t] ? KAO_STATUS_INFEASIBLE_PROVEN : KAO_STATUS_NO_FEASIBLE; r.objective = -1; }
        else r.status = r.objective >= r.upper_bound ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
    }
    return KAO_OK;
}

int kao_session_stats(kao_session *s, kao_stats *out) {
    if (!s || !out) return fail(KAO_ERR_INVALID, "null argument");
    int rc = kao_session_sync(s);
    if (rc) return rc;
    std::memset(out, 0, sizeof *out);
    out->launches = s->launch;
    out->delta_candidates = s->delta_total;
    out->full_candidates = (uint64_t)s->launch * (uint64_t)s->total_restarts;
    out->ms_search = s->ms_search; out->ms_eval = s->ms_eval;
    out->search_bytes_algo = s->search_bytes_total;
    out->eval_bytes_algo = s->eval_bytes_per_launch * s->launch;
    out->n_restarts_total = s->total_restarts;
    for (const kao_session::LaunchGroup &g : s->groups)
        out->lds_bytes_search = std::max(out->lds_bytes_search, (int32_t)search_lds_bytes(g.maxP, g.maxBx, g.waves, g.global_a, s->priced, g.nw, s->any_bw, g.maxR, g.team, g.cur_global));
    out->launch_groups = (int32_t)s->groups.size();
    out->blocks_search = s->blocks_search;
    out->search_rf3_launches = (int32_t)std::min<uint64_t>(s->search_rf3_launches, (uint64_t)INT32_MAX);
    HIP_TRY(hipMemcpy(&out->drift, s->d_drift, 4, hipMemcpyDeviceToHost));
    return KAO_OK;
}

int kao_session_chunked_launches(kao_session *s, int64_t *out) {
    if (!s || !out) return fail(KAO_ERR_INVALID, "null argument");
    *out = (int64_t)s->search_chunked_launches;
    return KAO_OK;
}

int kao_session_small_launches(kao_session *s, int64_t *out) {
    if (!s || !out) return fail(KAO_ERR_INVALID, "null argument");
    *out = (int64_t)s->search_small_launches;
    return KAO_OK;
}

int kao_session_restart_state(kao_session *s, int32_t topic, int32_t restart, uint16_t *final_state, uint16_t *best_state,
                              int32_t info[4]) {
    if (!s || topic < 0 || topic >= s->n_topics) return fail(KAO_ERR_INVALID, "bad topic");
    const PreparedTopic &pt = s->pts[(size_t)topic];
    const TopicDev &d = pt.d;
    if (restart < 0 || restart >= d.n_restarts) return fail(KAO_ERR_INVALID, "bad restart");
    HIP_TRY(hipSetDevice(s->device));
    int rc = kao_session_sync(s);
    if (rc) return rc;
    if (final_state) {
        const bool ga = s->topic_global[(size_t)topic] != 0;
        const int nw = d.nw;
        std::vector<uint16_t> raw((size_t)d.P * nw * (ga ? 2 : 1));   // global path: nw words per partition; LDS path: nw x u16
        HIP_TRY(hipMemcpy(raw.data(), s->d_state + d.state_off + (uint64_t)restart * d.P * nw * (ga ? 4 : 2), raw.size() * 2, hipMemcpyDeviceToHost));
        for (int p = 0; p < d.P; ++p)
            for (int k = 0; k < d.RF; ++k) {
                // global path: word = x | rack << 16 (little endian: x is the low half; none = all ones); LDS path: the index itself
                const uint16_t x = ga ? raw[((size_t)p * nw + k) * 2] : raw[(size_t)p * nw + k];
                final_state[(size_t)p * d.RF + k] = x < pt.ext_of.size() ? pt.ext_of[x] : (uint16_t)KAO_NONE;
            }
    }
    if (best_state)
        HIP_TRY(hipMemcpy(best_state, s->d_best + d.best_off + (uint64_t)restart * d.P * d.RF, (size_t)d.P * d.RF * 2, hipMemcpyDeviceToHost));
    if (info) HIP_TRY(hipMemcpy(info, s->d_info + (size_t)(d.restart_base + restart) * 4, 16, hipMemcpyDeviceToHost));
    return KAO_OK;
}

}  // extern "C"

namespace kao {

// the topic's winning assignment (dense [P*RF]) as of the last finished launch
int session_topic_best(kao_session *s, int i, uint16_t *out) {
    HIP_TRY(hipSetDevice(s->device));
    launch_gather(s->d_topics, s->n_topics, s->d_keys, s->d_best, s->d_viol, s->d_win_assign, s->d_win_viol, s->stream);
    HIP_TRY(hipGetLastError());
    const TopicDev &d = s->pts[(size_t)i].d;
    HIP_TRY(hipMemcpyAsync(out, s->d_win_assign + d.win_off, (size_t)d.P * d.RF * 2, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return KAO_OK;
}
// every restart's best feasible objective (-1: never feasible) and one restart's best snapshot (dense [P*RF]) as of the last
// finished launch: the starting points of kao_solve's further KAO-CX runs
int session_restart_objs(kao_session *s, int i, std::vector<int32_t> &objs) {
    HIP_TRY(hipSetDevice(s->device));
    const TopicDev &d = s->pts[(size_t)i].d;
    std::vector<int32_t> info((size_t)d.n_restarts * 4);
    HIP_TRY(hipMemcpyAsync(info.data(), s->d_info + (size_t)d.restart_base * 4, info.size() * 4, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    objs.resize((size_t)d.n_restarts);
    for (int r = 0; r < d.n_restarts; ++r) objs[(size_t)r] = info[(size_t)r * 4];
    return KAO_OK;
}
int session_restart_best(kao_session *s, int i, int restart, uint16_t *out) {
    HIP_TRY(hipSetDevice(s->device));
    const TopicDev &d = s->pts[(size_t)i].d;
    if (restart < 0 || restart >= d.n_restarts) return fail(KAO_ERR_INVALID, "bad restart");
    HIP_TRY(hipMemcpyAsync(out, s->d_best + d.best_off + (uint64_t)restart * d.P * d.RF, (size_t)d.P * d.RF * 2, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return KAO_OK;
}
// a feasible assignment found outside K-search (KAO-CX) becomes the topic's incumbent: winner buffer + packed key with the
// reserved restart id, exactly as an assignment adopted from another GPU (k_gather leaves it alone, elite launches re-seed from it)
int session_adopt_external(kao_session *s, int i, const uint16_t *assign, int64_t objective, uint64_t *key_out) {
    HIP_TRY(hipSetDevice(s->device));
    const TopicDev &d = s->pts[(size_t)i].d;
    const uint64_t key = ((uint64_t)((int64_t)kObjCap - objective) << 20) | (uint64_t)kExternalRestart;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_win_assign + d.win_off, assign, (size_t)d.P * d.RF * 2, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_keys + i, &key, 8, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    *key_out = key;
    return KAO_OK;
}

}  // namespace kao
