// kao_evalplan.cpp -- K-eval outside a session: evaluation plans (one topic resident on the device, batches of candidates scored by
// k_eval), kao_evaluate(_batch) on top of them, and the canonical tie-break (kao_canonicalize, k_canon).
#include <cstring>

#include "kao_host.h"

namespace {

template <typename T>
int dev_alloc_copy(T **dst, const std::vector<T> &src) {
    *dst = nullptr;
    const size_t n = std::max<size_t>(src.size(), 1);
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), n * sizeof(T)));
    if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return KAO_OK;
}

}  // namespace

extern "C" {

int kao_eval_plan_create(const kao_topic *t, kao_eval_plan **out) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    *out = nullptr;
    int rc = require_init();
    if (rc) return rc;
    kao_eval_plan *p = new kao_eval_plan();
    p->device = cur_device();
    rc = prepare(t, 0, p->pt);
    if (rc) { delete p; return rc; }
    p->cur_in_lds = eval_lds_bytes(p->pt.d.P, p->pt.d.B, true, p->pt.d.nw) <= kLdsLimit;
    if (eval_lds_bytes(p->pt.d.P, p->pt.d.B, p->cur_in_lds, p->pt.d.nw) > kLdsLimit) { delete p; return fail(KAO_ERR_UNSUPPORTED, "broker tables exceed 160 KiB of LDS"); }
    p->pt.d.best_off = 0; p->pt.d.rackof_off = 0; p->pt.d.curd_off = 0; p->pt.d.bwd_off = 0;
    std::vector<TopicDev> td(1, p->pt.d);
    if ((rc = dev_alloc_copy(&p->d_topic, td)) || (rc = dev_alloc_copy(&p->d_rackof, p->pt.rack_of)) ||
        (rc = dev_alloc_copy(&p->d_curd, p->pt.cur_dense)) || (p->pt.d.has_bw && (rc = dev_alloc_copy(&p->d_bwd, p->pt.bw_dense)))) { kao_eval_plan_destroy(p); return rc; }
    hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess && (int64_t)p->pt.d.P * p->pt.d.RF > 65535) {
        e = hipMalloc(reinterpret_cast<void **>(&p->d_overflow), 4);
        if (e == hipSuccess) e = hipMemset(p->d_overflow, 0, 4);
    }
    if (e == hipSuccess) e = hipEventCreate(&p->ev0);
    if (e == hipSuccess) e = hipEventCreate(&p->ev1);
    if (e != hipSuccess) { kao_eval_plan_destroy(p); return fail(KAO_ERR_HIP, std::string("kao_eval_plan_create: ") + hipGetErrorString(e)); }
    *out = p;
    return KAO_OK;
}

int kao_eval_plan_run(kao_eval_plan *p, const void *d_candidates, int64_t n, void *d_objective, void *d_violations,
                      void *d_best_key) {
    if (!p || !d_candidates || n < 1) return fail(KAO_ERR_INVALID, "bad plan/candidates");
    if (n > (1 << 20)) return fail(KAO_ERR_INVALID, "at most 2^20 candidates per run (packed key id width)");
    HIP_TRY(hipSetDevice(p->device));
    if (n != p->map_n) {
        // small batches of large candidates (KAO-CX: <= 513 assignments of up to 10^5 slots) spread over the compute units: one
        // candidate per wavefront instead of eight, as soon as 32 per workgroup would leave most of the chip idle
        int cpb = p->cands_per_block;
        const int64_t fill = 4 * (int64_t)std::max(num_cu(p->device), 1);
        if (n < fill * 8) cpb = (int)std::min<int64_t>(cpb, std::max<int64_t>(kWaves, ((n + fill - 1) / fill) * kWaves));
        p->coop = n <= fill && p->pt.d.P >= 1024;   // few large candidates: one workgroup each, its wavefronts cooperating
        if (p->coop) cpb = 1;
        const int nb = (int)((n + cpb - 1) / cpb);
        std::vector<int4> map((size_t)nb);
        for (int b = 0; b < nb; ++b) {
            const int first = b * cpb;
            map[b] = make_int4(0, first, (int)std::min<int64_t>(cpb, n - first), first);
        }
        p->map_n = -1;  // no valid map until the new one is uploaded
        if (p->d_map) { int4 *old_map = p->d_map; p->d_map = nullptr; HIP_TRY(hipFree(old_map)); }
        int rc = dev_alloc_copy(&p->d_map, map);
        if (rc) return rc;
        p->map_n = n;
        p->map_blocks = nb;
    }
    EvalPools pl{};
    pl.topics = p->d_topic; pl.block_map = p->d_map; pl.rackof_pool = p->d_rackof; pl.curd_pool = p->d_curd;
    pl.cand = static_cast<const uint16_t *>(d_candidates);
    pl.objective = static_cast<int32_t *>(d_objective);
    pl.violations = static_cast<int32_t *>(d_violations);
    pl.best_key = static_cast<unsigned long long *>(d_best_key);
    pl.maxP = p->pt.d.P; pl.maxB = p->pt.d.B; pl.cur_in_lds = p->cur_in_lds ? 1 : 0; pl.coop = p->coop ? 1 : 0; pl.rf_uniform = p->pt.d.RF;
    pl.overflow = p->d_overflow; pl.bwd_pool = p->d_bwd;
    HIP_TRY(hipEventRecord(p->ev0, p->stream));
    launch_eval(pl, p->map_blocks, p->pt.d.nw, p->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(p->ev1, p->stream));
    p->timed = true;
    return KAO_OK;
}

int kao_eval_plan_sync(kao_eval_plan *p, double *ms_last) {
    if (!p) return fail(KAO_ERR_INVALID, "null plan");
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (p->d_overflow) {
        int32_t flag = 0;
        HIP_TRY(hipMemcpy(&flag, p->d_overflow, 4, hipMemcpyDeviceToHost));
        if (flag) {
            HIP_TRY(hipMemset(p->d_overflow, 0, 4));
            return fail(KAO_ERR_UNSUPPORTED, "a candidate puts more than 65,535 replicas on one broker (16-bit per-broker counters)");
        }
    }
    if (ms_last) {
        float ms = 0;
        if (p->timed) HIP_TRY(hipEventElapsedTime(&ms, p->ev0, p->ev1));
        *ms_last = ms;
    }
    return KAO_OK;
}

void kao_eval_plan_destroy(kao_eval_plan *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    (void)hipFree(p->d_topic); (void)hipFree(p->d_rackof); (void)hipFree(p->d_curd); (void)hipFree(p->d_map); (void)hipFree(p->d_overflow); (void)hipFree(p->d_bwd);
    if (p->ev0) (void)hipEventDestroy(p->ev0);
    if (p->ev1) (void)hipEventDestroy(p->ev1);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

namespace {
// a plan plus growable device buffers, reused across batches (kao_canonicalize issues many small ones)
struct EvalCtx {
    kao_eval_plan *plan = nullptr;
    size_t per = 0, cap = 0;
    uint16_t *d_c = nullptr; int32_t *d_o = nullptr, *d_v = nullptr;
    ~EvalCtx() { (void)hipFree(d_c); (void)hipFree(d_o); (void)hipFree(d_v); kao_eval_plan_destroy(plan); }
    int open(const kao_topic *t) {
        per = (size_t)t->n_partitions * t->rf;
        return kao_eval_plan_create(t, &plan);
    }
    int run(const uint16_t *candidates, int64_t n, int32_t *objective, int32_t *violations) {
        const int64_t chunk_max = 1 << 20;
        for (int64_t done = 0; done < n; done += chunk_max) {
            const int64_t c = std::min(chunk_max, n - done);
            if ((size_t)c > cap) {
                (void)hipFree(d_c); (void)hipFree(d_o); (void)hipFree(d_v);
                d_c = nullptr; d_o = d_v = nullptr;
                cap = std::max<size_t>((size_t)c, std::min<size_t>(2 * cap + 64, (size_t)chunk_max));
                if (hipMalloc(reinterpret_cast<void **>(&d_c), cap * per * 2) != hipSuccess ||
                    hipMalloc(reinterpret_cast<void **>(&d_o), cap * 4) != hipSuccess ||
                    hipMalloc(reinterpret_cast<void **>(&d_v), cap * 32) != hipSuccess) { cap = 0; return fail(KAO_ERR_NOMEM, "hipMalloc"); }
            }
            HIP_TRY(hipMemcpy(d_c, candidates + (size_t)done * per, (size_t)c * per * 2, hipMemcpyHostToDevice));
            int rc = kao_eval_plan_run(plan, d_c, c, d_o, d_v, nullptr);
            if (!rc) rc = kao_eval_plan_sync(plan, nullptr);
            if (rc) return rc;
            HIP_TRY(hipMemcpy(objective + done, d_o, (size_t)c * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(violations + done * 8, d_v, (size_t)c * 32, hipMemcpyDeviceToHost));
        }
        return KAO_OK;
    }
};
}  // namespace

int kao_evaluate_batch(const kao_topic *t, const uint16_t *candidates, int64_t n, int32_t *objective, int32_t *violations) {
    if (!candidates || !objective || !violations || n < 1) return fail(KAO_ERR_INVALID, "null buffers");
    EvalCtx ctx;
    int rc = ctx.open(t);
    if (rc) return rc;
    return ctx.run(candidates, n, objective, violations);
}

int kao_evaluate(const kao_topic *t, const uint16_t *assignment, int64_t *objective, int32_t violations[8]) {
    int32_t obj = 0;
    int rc = kao_evaluate_batch(t, assignment, 1, &obj, violations);
    if (!rc && objective) *objective = obj;
    return rc;
}

int kao_canonicalize(const kao_topic *t, uint16_t *a) {
    if (!a) return fail(KAO_ERR_INVALID, "null assignment");
    if (t && (t->broker_w || t->broker_wl)) return KAO_OK;   // moving a replica to another broker changes the objective: nothing to canonicalise
    int rc = require_init();
    if (rc) return rc;
    PreparedTopic pt;
    if ((rc = prepare(t, 0, pt))) return rc;
    const TopicDev &d = pt.d;
    const int P = d.P, RF = d.RF, B = d.B;
    if (canon_lds_bytes(d.Bx) > kLdsLimit) return fail(KAO_ERR_UNSUPPORTED, "broker tables exceed 160 KiB of LDS");
    const int nw = d.nw;
    std::vector<uint32_t> cur_words((size_t)P * nw), a_words((size_t)P * nw, kNoneW);
    for (int p = 0; p < P; ++p) {
        const uint16_t *c = &pt.cur_int[(size_t)p * nw];
        for (int k = 0; k < nw; ++k) cur_words[(size_t)p * nw + k] = replica_word(c[k], d.m);
        for (int k = 0; k < RF; ++k) {
            const unsigned b = a[(size_t)p * RF + k];
            if (b >= (unsigned)B) return KAO_OK;  // an empty slot: infeasible, nothing to polish
            a_words[(size_t)p * nw + k] = replica_word(pt.int_of[b], d.m);
        }
    }
    // one device buffer: [TopicDev][status 16 B][cur words][A words][ext][rsz]
    const size_t wbytes = (size_t)P * nw * 4;
    const size_t o_status = align_up(sizeof(TopicDev)), o_cur = o_status + 256, o_a = o_cur + align_up(wbytes);
    const size_t o_ext = o_a + align_up(wbytes), o_rsz = o_ext + align_up(pt.ext_of.size() * 2);
    const size_t total = o_rsz + align_up(pt.rack_size.size() * 4);
    std::vector<unsigned char> stage(total, 0);
    std::memcpy(stage.data(), &d, sizeof(TopicDev));
    std::memcpy(stage.data() + o_cur, cur_words.data(), wbytes);
    std::memcpy(stage.data() + o_a, a_words.data(), wbytes);
    std::memcpy(stage.data() + o_ext, pt.ext_of.data(), pt.ext_of.size() * 2);
    std::memcpy(stage.data() + o_rsz, pt.rack_size.data(), pt.rack_size.size() * 4);
    void *dev = nullptr; size_t cap = 0;
    if ((rc = arena_get(total, &dev, &cap))) return rc;
    unsigned char *db = static_cast<unsigned char *>(dev);
    hipStream_t st = nullptr;
    if ((rc = stream_get(&st))) { arena_put(dev, cap, cur_device()); return rc; }
    int32_t status[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(db, stage.data(), total, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        launch_canon(reinterpret_cast<const TopicDev *>(db), reinterpret_cast<const uint32_t *>(db + o_cur),
                     reinterpret_cast<const uint16_t *>(db + o_ext), reinterpret_cast<const int32_t *>(db + o_rsz),
                     reinterpret_cast<uint32_t *>(db + o_a), d.Bx, nw, reinterpret_cast<int32_t *>(db + o_status), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(a_words.data(), db + o_a, wbytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(status, db + o_status, sizeof status, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    stream_put(st, cur_device());
    arena_put(dev, cap, cur_device());
    if (e != hipSuccess) return fail(KAO_ERR_HIP, std::string("kao_canonicalize: ") + hipGetErrorString(e));
    if (!status[0]) return KAO_OK;  // only feasible assignments are polished
    for (int p = 0; p < P; ++p) {
        for (int k = 0; k < RF; ++k) a[(size_t)p * RF + k] = pt.ext_of[a_words[(size_t)p * nw + k] & 0xFFFFu];
    }
    for (int p = 0; p < P; ++p) {  // followers: retained ones in their current order, then new ones ascending
        std::vector<uint16_t> fol(a + (size_t)p * RF + 1, a + (size_t)p * RF + RF), kept, fresh;
        for (int k = 0; k < t->rf_cur; ++k) {
            const uint16_t c = t->current[(size_t)p * t->rf_cur + k];
            if (std::find(fol.begin(), fol.end(), c) != fol.end() && std::find(kept.begin(), kept.end(), c) == kept.end()) kept.push_back(c);
        }
        for (uint16_t f : fol) if (std::find(kept.begin(), kept.end(), f) == kept.end()) fresh.push_back(f);
        std::sort(fresh.begin(), fresh.end());
        kept.insert(kept.end(), fresh.begin(), fresh.end());
        std::copy(kept.begin(), kept.end(), a + (size_t)p * RF + 1);
    }
    return KAO_OK;
}

}  // extern "C"
