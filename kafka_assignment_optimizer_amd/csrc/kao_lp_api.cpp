// kao_lp_api.cpp -- the one-shot KAO-LP entry points of the C ABI on top of kao_lp.hip (the solve) and kao_round.cpp (the rounding):
// kao_lp_bound, kao_lp_round, kao_lp_round_host, kao_lp_trace.
#include <cstring>

#include "kao_host.h"

extern "C" {

int kao_lp_bound(const kao_topic *t, double tol, int32_t max_iters, int64_t *bound, int64_t *best_dual, int32_t *multipliers, double stats[8]) {
    if (!t) return fail(KAO_ERR_INVALID, "null topic");
    int rc = require_init();
    if (rc) return rc;
    LpCtx *lp = nullptr;
    if ((rc = lp_open(t, &lp))) return rc;
    std::vector<int32_t> mult(2 * (size_t)t->n_brokers + (size_t)t->n_racks);
    rc = lp_solve(lp, tol > 0 ? tol : 1e-7, max_iters > 0 ? max_iters : 80, mult.data(), stats, nullptr);
    lp_close(lp);
    if (rc) return rc;
    if (multipliers) std::memcpy(multipliers, mult.data(), mult.size() * 4);
    // the dual value at those multipliers, in integers: one K-bound iteration from them
    SessionPtr s;
    if ((rc = bound_only_session(t, s))) return rc;
    if ((rc = kao_session_set_dual_state(s.get(), 0, mult.data(), mult.data() + t->n_brokers, mult.data() + 2 * (size_t)t->n_brokers))) return rc;
    const int64_t target = 0;
    int32_t fl = 0, itn = 0;
    int64_t bd = 0;
    if ((rc = kao_session_bound_step(s.get(), &target, 1)) || (rc = kao_session_bounds(s.get(), nullptr, &fl, &itn)) ||
        (rc = kao_session_dual_state(s.get(), 0, nullptr, nullptr, nullptr, &bd))) return rc;
    if (best_dual) *best_dual = bd;
    if (bound) *bound = dual_bound_value(fl, itn, bd);
    return KAO_OK;
}

int kao_lp_round(const kao_topic *t, double pert, uint32_t salt, double tol, int32_t max_iters, int32_t use_fallback, uint16_t *assignment,
                 int64_t *objective, int32_t violations[8], double stats[8]) {
    if (!t || !assignment) return fail(KAO_ERR_INVALID, "null topic / assignment");
    int rc = require_init();
    if (rc) return rc;
    LpCtx *lp = nullptr;
    if ((rc = lp_open(t, &lp))) return rc;
    const size_t slots = (size_t)t->n_partitions * t->rf;
    const double eps = pert > 0 ? pert : lp_default_pert(t);
    double st[8] = {0};
    rc = lp_solve(lp, tol > 0 ? tol : 1e-8, max_iters > 0 ? max_iters : 150, nullptr, st, nullptr, eps, salt);
    std::vector<uint8_t> q((size_t)(2 * t->rf_cur + 2 * t->n_racks) * t->n_partitions);
    std::vector<int32_t> zq(2 * (size_t)t->n_brokers);
    if (!rc) rc = lp_primal(lp, q.data(), zq.data());
    lp_close(lp);
    if (rc) return rc;
    const double t0 = now_s();
    std::vector<uint16_t> fb;
    if (use_fallback) fb.assign(assignment, assignment + slots);
    int32_t rep[4] = {0, 0, 0, 0};
    if ((rc = lp_round_assignment(t, q.data(), zq.data(), use_fallback ? fb.data() : nullptr, assignment, rep))) return rc;
    const double t1 = now_s();
    int64_t obj = 0;
    int32_t viol[8] = {0};
    if ((rc = kao_evaluate(t, assignment, &obj, viol))) return rc;
    if (objective) *objective = obj;
    if (violations) std::memcpy(violations, viol, sizeof viol);
    if (stats) { stats[0] = st[0]; stats[1] = st[3]; stats[2] = rep[0]; stats[3] = rep[1] + rep[2]; stats[4] = rep[3]; stats[5] = st[7]; stats[6] = (t1 - t0) * 1e3; stats[7] = eps; }
    return KAO_OK;
}

int kao_lp_round_host(const kao_topic *t, const uint8_t *q, const int32_t *zq, int32_t use_fallback, uint16_t *assignment, int32_t rep[4]) {
    if (!t || !assignment || (use_fallback != 2 && (!q || !zq))) return fail(KAO_ERR_INVALID, "null argument");
    int rc = validate(t);
    if (rc) return rc;
    if (use_fallback == 2) {   // the band repair alone on the assignment passed in
        if (rep) rep[0] = rep[1] = rep[2] = rep[3] = 0;
        for (size_t i = 0, n = (size_t)t->n_partitions * t->rf; i < n; ++i)
            if (assignment[i] >= t->n_brokers) return fail(KAO_ERR_INVALID, "repair: a complete assignment expected");
        return lp_round_assignment(t, nullptr, zq, nullptr, assignment, rep);
    }
    std::vector<uint16_t> fb;
    if (use_fallback) fb.assign(assignment, assignment + (size_t)t->n_partitions * t->rf);
    return lp_round_assignment(t, q, zq, use_fallback ? fb.data() : nullptr, assignment, rep);
}

int kao_lp_trace(const kao_topic *t, double tol, int32_t max_iters, double *trace, double stats[8], int32_t *multipliers) {
    if (!t) return fail(KAO_ERR_INVALID, "null topic");
    int rc = require_init();
    if (rc) return rc;
    LpCtx *lp = nullptr;
    if ((rc = lp_open(t, &lp))) return rc;
    double pert = env_real("KAO_LP_TRACE_PERT", 0.0);   // experiment hook KAO_LP_TRACE_PERT=<eps> (-1: the solve's own default): the trace of the PERTURBED solve
    if (pert < 0) pert = std::min(1e-4, 1.5 / ((double)t->n_partitions * t->rf));
    rc = lp_solve(lp, tol > 0 ? tol : 1e-7, max_iters > 0 ? max_iters : 80, multipliers, stats, trace, pert, 0);
    lp_close(lp);
    return rc;
}

}  // extern "C"
