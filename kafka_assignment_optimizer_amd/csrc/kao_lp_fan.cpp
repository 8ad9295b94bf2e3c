// kao_lp_fan.cpp -- ONE LP over several devices (round 6): the collective side of kao_lp.hip's shards, and a test hook
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include "kao_rccl.h"

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
        DeviceScope on(devs[(size_t)r]);   // for the thread's life
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
        DeviceScope on(devs[(size_t)r]);
        int e = on.rc;
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
    std::vector<std::thread> th;
    for (int r = 1; r < n_dev; ++r) th.emplace_back(work, r);
    work(0);
    for (std::thread &x : th) x.join();
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
}  // extern "C"
