// kao_session_bound.cpp -- K-bound on a session: the launches on the session's own priority stream, the search prices they export, the
// bounds and the dual state read back, and kao_dual_bound (K-bound alone on a throw-away session).
#include <cstring>

#include "kao_host.h"

namespace {

// K-bound's own stream, highest priority: a K-bound launch is a handful of workgroups that should not queue behind a full K-search grid
int ensure_bound_stream(kao_session *s) {
    if (s->stream_bound) return KAO_OK;
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&s->stream_bound, hipStreamNonBlocking, hi));
    HIP_TRY(hipEventCreate(&s->ev_bound0));
    HIP_TRY(hipEventCreate(&s->ev_bound1));
    return KAO_OK;
}

// K-bound state is initialised by its first user only (most sessions never need K-bound): multipliers and directions 0, best dual
// value "infinite" (kDualNone), info 0
int ensure_dual_state(kao_session *s) {
    if (s->dual_state_init) return KAO_OK;
    HIP_TRY(hipMemsetAsync(s->d_dual, 0, s->dual_bytes, s->stream_bound));
    HIP_TRY(hipMemsetAsync(s->d_dual_rb, 0x7F, (size_t)s->n_topics * 8, s->stream_bound));
    HIP_TRY(hipMemsetAsync(s->d_dual_rb + (size_t)s->n_topics * 8, 0, (size_t)s->n_topics * 16, s->stream_bound));
    s->dual_state_init = true;
    return KAO_OK;
}

// How one class of topics (`ids`: RF and current RF <= 4, or 5..8) is launched: the LDS carve (into `bp`), the wavefronts of k_bound's
// one workgroup per topic, whether the persistent driver may be used; returns the partitions per slice of the sliced drivers
// (k_bound_multi / k_bound_step), or 0 for k_bound
int plan_class_launch(const kao_session *s, const int32_t *ids, int n, BoundPools &bp, int &waves, bool &multi) {
    int maxB = 0, maxP = 0, maxR = 0;
    for (int i = 0; i < n; ++i) {
        const TopicDev &d = s->pts[(size_t)ids[i]].d;
        maxB = std::max(maxB, d.B); maxP = std::max(maxP, d.P); maxR = std::max(maxR, d.R);
    }
    bp.maxB = maxB; bp.maxP = maxP; bp.maxR = maxR;
    bp.cur_in_lds = bound_lds_bytes(maxB, maxP, maxR, true, bp.ne, bp.bwd_pool != nullptr) <= kLdsLimit ? 1 : 0;
    // lanes own partitions, wavefronts own racks when the pools are rebuilt: enough wavefronts for either, at most 16
    waves = std::min(16, std::max({1, (maxP + 63) / 64, std::min(maxR, 8)}));
    // topics beyond a few thousand partitions: one iteration per launch, the partitions sliced over several workgroups
    // (k_bound_step); a launch that holds such a topic runs all its topics that way.  KAO_BOUND_CHUNK = partitions per
    // slice (test hook: small values slice small topics)
    int chunk = maxP > 2048 ? 512 : 0;
    // Round 3: the sliced topics run on the PERSISTENT multi-workgroup driver (k_bound_multi) -- and so do topics from 1,024
    // partitions up, in slices of 512 (a 2,000-partition topic: 52 us per iteration in k_bound's one workgroup).  Its workgroups
    // wait for each other, so a launch is kept to 96 of them (larger slices otherwise).  KAO_BOUND_MULTI=0: the round-2 drivers.
    multi = env_int("KAO_BOUND_MULTI", 1) != 0 && !s->multi_off;
    if (multi && chunk == 0 && maxP >= 1024) chunk = 512;
    chunk = (int)std::max<int64_t>(0, env_int("KAO_BOUND_CHUNK", chunk)) / 64 * 64;
    if (multi && chunk > 0) {   // workgroups that wait for others (topics of more than one slice): at most 96 per launch
        auto waiting_at = [&](int c) {
            int64_t nb = 0;
            for (int i = 0; i < n; ++i) { const int sl = (s->pts[(size_t)ids[i]].d.P + c - 1) / c; nb += sl > 1 ? sl : 0; }
            return nb;
        };
        while (chunk < (1 << 20) && waiting_at(chunk) > 96) chunk += chunk;
    }
    return chunk;
}

// force_step: the launch repeats one that k_bound_multi gave up on (flag 16): the one-iteration-per-launch kernels, from the same state
int bound_step(kao_session *s, const int64_t *target, int32_t iters, bool force_step) {
    if (!s || !target) return fail(KAO_ERR_INVALID, "null argument");
    if (iters < 1) return fail(KAO_ERR_INVALID, "iters < 1");
    HIP_TRY(hipSetDevice(s->device));
    // the previous launch's H2D copies read the staging vectors below: wait for them before rewriting
    if (s->stream_bound) HIP_TRY(hipStreamSynchronize(s->stream_bound));
    s->h_dual_ids.clear();
    s->h_dual_target.assign((size_t)s->n_topics, -1);
    // two classes of topics, one launch each: RF and current RF <= 4 (k_bound<4>), RF 5..8 (k_bound<8>); ids of the first class first
    auto wide_slots = [&](int t) { return s->pts[(size_t)t].d.RF > kRFP || s->pts[(size_t)t].d.rf_cur > kRFP; };
    int n_class[2] = {0, 0};
    for (int cls = 0; cls < 2; ++cls)
        for (int t = 0; t < s->n_topics; ++t) {
            if (target[t] < 0 || !s->dual_ok[(size_t)t] || s->topic_infeasible[(size_t)t] || (int)wide_slots(t) != cls) continue;
            if (target[t] > (int64_t)1 << 40) return fail(KAO_ERR_INVALID, "target out of range");
            s->h_dual_ids.push_back(t);
            s->h_dual_target[(size_t)t] = target[t];
            n_class[cls]++;
        }
    if (s->h_dual_ids.empty()) return KAO_OK;
    int rc = ensure_bound_stream(s);
    if (rc) return rc;
    // one K-bound launch in flight at a time (it continues from the state the previous one left in HBM); the session
    // upload was synchronised at creation, K-search and K-bound share read-only tables only
    HIP_TRY(hipStreamSynchronize(s->stream_bound));
    if ((rc = ensure_dual_state(s))) return rc;
    // pageable staging: hipMemcpyAsync returns once the host buffers have been consumed
    HIP_TRY(hipMemcpyAsync(s->d_dual_target, s->h_dual_target.data(), (size_t)s->n_topics * 8, hipMemcpyHostToDevice, s->stream_bound));
    HIP_TRY(hipMemcpyAsync(s->d_dual_ids, s->h_dual_ids.data(), s->h_dual_ids.size() * 4, hipMemcpyHostToDevice, s->stream_bound));
    BoundPools bp{};
    bp.topics = s->d_topics; bp.ids = s->d_dual_ids; bp.rackof_pool = s->d_rackof; bp.curd_pool = s->d_curd;
    bp.dual_pool = s->d_dual; bp.target = s->d_dual_target;
    bp.best_L = reinterpret_cast<long long *>(s->d_dual_rb);
    bp.info = reinterpret_cast<int32_t *>(s->d_dual_rb + (size_t)s->n_topics * 8);
    bp.ext_pool = s->d_ext; bp.rsz_pool = s->d_rsz;
    bp.iters = iters;
    bp.bwd_pool = s->any_bw ? s->d_bwd : nullptr;
    // K-search launches already enqueued may still read the half this launch is about to overwrite -- except under kao_solve's
    // deterministic schedule, which starts K-bound only when the enqueued K-search launches read the OTHER half (the launch
    // that read this one has been waited for)
    if (s->priced && !s->bound_no_wait) {
        if (!s->ev_search) HIP_TRY(hipEventCreateWithFlags(&s->ev_search, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(s->ev_search, s->stream));
        HIP_TRY(hipStreamWaitEvent(s->stream_bound, s->ev_search, 0));
    }
    // prices go into the half K-search is NOT reading; kao_session_adopt_prices flips the halves once this launch is done
    const int wh = s->price_read ^ 1;
    if (s->price_write_last >= 0 && s->price_write_last != wh)  // keep the prices of topics this launch does not cover
        HIP_TRY(hipMemcpyAsync(s->d_price + (size_t)wh * s->price_half_i32, s->d_price + (size_t)(wh ^ 1) * s->price_half_i32,
                               s->price_half_i32 * 4, hipMemcpyDeviceToDevice, s->stream_bound));
    bp.price_pool = s->d_price + (size_t)wh * s->price_half_i32;
    bp.export_prices = 1;
    s->price_write_last = wh;
    HIP_TRY(hipEventRecord(s->ev_bound0, s->stream_bound));
    s->h_wide_map.clear();
    for (int cls = 0, first = 0; cls < 2; first += n_class[cls], ++cls) {
        const int n = n_class[cls];
        if (!n) continue;
        const int32_t *ids = s->h_dual_ids.data() + first;
        bp.ids = s->d_dual_ids + first;
        bp.ne = cls ? 8 : 4;
        int waves = 1;
        bool multi = false;
        const int chunk = plan_class_launch(s, ids, n, bp, waves, multi);
        launch_bound_center(bp, n, s->stream_bound);   // exact line search along the common shift of every family
        if (chunk == 0) { launch_bound(bp, n, waves, s->stream_bound); continue; }
        const size_t map0 = s->h_wide_map.size();
        for (int i = 0; i < n; ++i)
            for (int sl = 0, nsl = (s->pts[(size_t)ids[i]].d.P + chunk - 1) / chunk; sl < nsl; ++sl) s->h_wide_map.push_back(make_int2(ids[i], sl));
        const int n_slices = (int)(s->h_wide_map.size() - map0);
        BoundWide wd{};
        wd.map = reinterpret_cast<const int2 *>(s->d_dual + s->wide_map_i32) + map0;
        wd.cnt_pool = s->d_dual;
        wd.ctl = reinterpret_cast<long long *>(s->d_dual + s->wide_ctl_i32);
        wd.chunk = chunk;
        HIP_TRY(hipMemcpyAsync(s->d_dual + s->wide_map_i32 + 2 * map0, s->h_wide_map.data() + map0, (size_t)n_slices * sizeof(int2),
                               hipMemcpyHostToDevice, s->stream_bound));
        // 16 wavefronts whatever the slice: the O(B) phases every workgroup repeats (pools, totals, band terms, step) are what
        // an iteration waits for (measured: slices of 256 with 4 wavefronts 32 us, slices of 512 with 8 wavefronts 19 us at 500 x 5,000)
        if (!(multi && !force_step && launch_bound_multi(bp, wd, n, n_slices, 16, s->stream_bound)))
            launch_bound_wide(bp, wd, n, n_slices, 16, s->stream_bound);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev_bound1, s->stream_bound));
    s->bound_inflight = true;
    s->bound_iters_last = iters;
    s->bound_launches++;
    return KAO_OK;
}

}  // namespace

namespace kao {
int bound_only_session(const kao_topic *t, SessionPtr &out) {
    kao_opts o{};
    o.restarts = kWaves;  // no search is run: the smallest session there is
    kao_session *raw = nullptr;
    const int rc = kao_session_create(t, 1, &o, &raw);
    out.reset(raw);
    if (rc) return rc;
    return out->dual_ok[0] ? KAO_OK : fail(KAO_ERR_UNSUPPORTED, "topic outside K-bound's limits");
}
}  // namespace kao

extern "C" {

int kao_session_bound_step(kao_session *s, const int64_t *target, int32_t iters) { return bound_step(s, target, iters, false); }

int kao_session_set_prices(kao_session *s, int32_t topic, const int32_t *a, const int32_t *l, const int32_t *g) {
    if (!s || topic < 0 || topic >= s->n_topics || !a || !l || !g) return fail(KAO_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    const TopicDev &d = s->pts[(size_t)topic].d;
    std::vector<int32_t> buf(2 * (size_t)d.B + kRackTab, 0);
    std::memcpy(buf.data(), a, (size_t)d.B * 4);
    std::memcpy(buf.data() + d.B, l, (size_t)d.B * 4);
    std::memcpy(buf.data() + 2 * (size_t)d.B, g, (size_t)d.R * 4);
    // both halves, so that a later adopt (which flips them) keeps host-set prices of topics K-bound does not cover
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->stream_bound) HIP_TRY(hipStreamSynchronize(s->stream_bound));
    for (int h = 0; h < 2; ++h)
        HIP_TRY(hipMemcpy(s->d_price + (size_t)h * s->price_half_i32 + d.price_off, buf.data(), buf.size() * 4, hipMemcpyHostToDevice));
    s->priced = true;
    return KAO_OK;
}

int kao_session_prices(kao_session *s, int32_t topic, int32_t *a, int32_t *l, int32_t *g) {
    if (!s || topic < 0 || topic >= s->n_topics) return fail(KAO_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    const TopicDev &d = s->pts[(size_t)topic].d;
    const int32_t *base = s->d_price + (size_t)s->price_read * s->price_half_i32 + d.price_off;
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (a) HIP_TRY(hipMemcpy(a, base, (size_t)d.B * 4, hipMemcpyDeviceToHost));
    if (l) HIP_TRY(hipMemcpy(l, base + d.B, (size_t)d.B * 4, hipMemcpyDeviceToHost));
    if (g) HIP_TRY(hipMemcpy(g, base + 2 * (size_t)d.B, (size_t)d.R * 4, hipMemcpyDeviceToHost));
    return KAO_OK;
}

int kao_session_adopt_prices(kao_session *s) {
    if (!s) return fail(KAO_ERR_INVALID, "null session");
    if (s->price_write_last < 0) return KAO_OK;  // K-bound has not run: nothing to adopt
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream_bound));
    s->price_read = s->price_write_last;
    s->priced = true;
    return KAO_OK;
}

int kao_session_bound_busy(kao_session *s) {
    if (!s) return fail(KAO_ERR_INVALID, "null session");
    HIP_TRY(hipSetDevice(s->device));
    if (!s->bound_inflight) return 0;
    const hipError_t e = hipEventQuery(s->ev_bound1);
    if (e == hipErrorNotReady) return 1;
    if (e != hipSuccess) return fail(KAO_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
    return 0;
}

int kao_session_bounds(kao_session *s, int64_t *upper_bound, int32_t *flags, int32_t *iters) {
    if (!s) return fail(KAO_ERR_INVALID, "null session");
    HIP_TRY(hipSetDevice(s->device));
    if (s->bound_launches) {
        std::vector<unsigned char> rb(s->dual_rb_bytes);
        HIP_TRY(hipMemcpyAsync(rb.data(), s->d_dual_rb, s->dual_rb_bytes, hipMemcpyDeviceToHost, s->stream_bound));
        HIP_TRY(hipStreamSynchronize(s->stream_bound));
        if (s->bound_inflight) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, s->ev_bound0, s->ev_bound1) == hipSuccess) s->bound_ms_last = ms;
            s->bound_inflight = false;
        }
        const int64_t *best = reinterpret_cast<const int64_t *>(rb.data());
        const int32_t *info = reinterpret_cast<const int32_t *>(rb.data() + (size_t)s->n_topics * 8);
        bool gave_up = false;
        for (int t = 0; t < s->n_topics; ++t) gave_up |= s->dual_ok[(size_t)t] && (info[t * 4 + 1] & 16);
        if (gave_up && !s->multi_off) {
            // k_bound_multi could not get a topic's workgroups resident together and committed nothing: the same launch again on
            // the kernels that do not wait for each other, and no further use of the persistent driver in this session
            // Only the topics that carry flag 16 run again: the others of the launch have committed their iterations (the abort
            // mark is all-or-nothing per topic, kao_bound.hip).  All drivers share one arithmetic, so the repeated topics end in
            // the state the persistent driver would have reached: the answer does not depend on whether a launch gave up.
            s->multi_off = true;
            std::vector<int64_t> again = s->h_dual_target;
            for (int t = 0; t < s->n_topics; ++t)
                if (!(s->dual_ok[(size_t)t] && (info[t * 4 + 1] & 16))) again[(size_t)t] = -1;
            int rc = bound_step(s, again.data(), s->bound_iters_last, true);
            if (rc) return rc;
            return kao_session_bounds(s, upper_bound, flags, iters);
        }
        for (int t = 0; t < s->n_topics; ++t) {
            if (!s->dual_ok[(size_t)t]) continue;
            s->dual_iters[(size_t)t] = info[t * 4 + 0];
            s->dual_flags[(size_t)t] = info[t * 4 + 1];
            if (best[t] < kDualNone) s->ub[(size_t)t] = std::min(s->ub[(size_t)t], dual_bound_value(info[t * 4 + 1], info[t * 4 + 0], best[t]));
        }
    }
    for (int t = 0; t < s->n_topics; ++t) {
        if (upper_bound) upper_bound[t] = s->ub[(size_t)t];
        if (flags) flags[t] = s->dual_flags[(size_t)t];
        if (iters) iters[t] = s->dual_iters[(size_t)t];
    }
    return KAO_OK;
}

int kao_session_dual_state(kao_session *s, int32_t topic, int32_t *a, int32_t *l, int32_t *g, int64_t *best_dual) {
    if (!s || topic < 0 || topic >= s->n_topics) return fail(KAO_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(s->device));
    const TopicDev &d = s->pts[(size_t)topic].d;
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->stream_bound) HIP_TRY(hipStreamSynchronize(s->stream_bound));
    const int32_t *base = s->d_dual + d.dual_off;
    if (!s->dual_state_init) {  // no K-bound launch yet: the initial state
        if (a) std::memset(a, 0, (size_t)d.B * 4);
        if (l) std::memset(l, 0, (size_t)d.B * 4);
        if (g) std::memset(g, 0, (size_t)d.R * 4);
        if (best_dual) *best_dual = kDualNone;
        return KAO_OK;
    }
    if (a) HIP_TRY(hipMemcpy(a, base, (size_t)d.B * 4, hipMemcpyDeviceToHost));
    if (l) HIP_TRY(hipMemcpy(l, base + d.B, (size_t)d.B * 4, hipMemcpyDeviceToHost));
    if (g) HIP_TRY(hipMemcpy(g, base + 4 * (size_t)d.B, (size_t)d.R * 4, hipMemcpyDeviceToHost));
    if (best_dual) HIP_TRY(hipMemcpy(best_dual, s->d_dual_rb + (size_t)topic * 8, 8, hipMemcpyDeviceToHost));
    return KAO_OK;
}

int kao_session_set_dual_state(kao_session *s, int32_t topic, const int32_t *a, const int32_t *l, const int32_t *g) {
    if (!s || topic < 0 || topic >= s->n_topics || !a || !l || !g) return fail(KAO_ERR_INVALID, "bad argument");
    if (!s->dual_ok[(size_t)topic]) return fail(KAO_ERR_UNSUPPORTED, "topic outside K-bound's limits");
    HIP_TRY(hipSetDevice(s->device));
    int rc = ensure_bound_stream(s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream_bound));
    if ((rc = ensure_dual_state(s))) return rc;
    const TopicDev &d = s->pts[(size_t)topic].d;
    // dual_pool: a[B] l[B] da[B] dl[B] g[kRackTab] dg[kRackTab] lv[8] ...: iterate replaced, direction memory and level control cleared
    std::vector<int32_t> buf(4 * (size_t)d.B + 2 * kRackTab + 8, 0);
    auto clampm = [](int32_t v) { return std::max(-kDualClamp, std::min(kDualClamp, v)); };
    for (int b = 0; b < d.B; ++b) { buf[(size_t)b] = clampm(a[b]); buf[(size_t)d.B + b] = clampm(l[b]); }
    for (int r = 0; r < d.R; ++r) buf[4 * (size_t)d.B + r] = clampm(g[r]);
    HIP_TRY(hipMemcpyAsync(s->d_dual + d.dual_off, buf.data(), buf.size() * 4, hipMemcpyHostToDevice, s->stream_bound));
    HIP_TRY(hipStreamSynchronize(s->stream_bound));
    return KAO_OK;
}

int kao_dual_bound(const kao_topic *t, int64_t target, int32_t iters, int32_t launches, int64_t *bound, int64_t *best_dual,
                   int32_t *iters_done, int32_t *flags, int32_t *multipliers) {
    if (!t) return fail(KAO_ERR_INVALID, "null topic");
    if (target < 0 || iters < 1 || launches < 1) return fail(KAO_ERR_INVALID, "bad target / iters / launches");
    SessionPtr s;
    int rc = bound_only_session(t, s);
    if (rc) return rc;
    int32_t fl = 0, itn = 0;
    for (int i = 0; i < launches; ++i) {
        if ((rc = kao_session_bound_step(s.get(), &target, iters)) || (rc = kao_session_bounds(s.get(), nullptr, &fl, &itn))) return rc;
        if (fl & 7) break;
    }
    int64_t bd = 0;
    if ((rc = kao_session_dual_state(s.get(), 0, multipliers, multipliers ? multipliers + t->n_brokers : nullptr,
                                     multipliers ? multipliers + 2 * (size_t)t->n_brokers : nullptr, &bd))) return rc;
    if (best_dual) *best_dual = bd;
    if (bound) *bound = dual_bound_value(fl, itn, bd);
    if (iters_done) *iters_done = itn;
    if (flags) *flags = fl;
    return KAO_OK;
}

}  // extern "C"
