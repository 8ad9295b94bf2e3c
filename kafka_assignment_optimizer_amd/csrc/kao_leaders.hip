// kao_leaders.hip -- kao_balance_leaders: the fewest preferred-leader changes that put every broker inside the leader band, replica
// sets kept.  Kernels and the C entry point.
//
// With the replica sets fixed the README model is a min-cost flow: partition p sends one unit to the broker it picks as leader
// (cost 0 for slot 0, 1 for any other slot), broker b passes f(b) in [lo, hi] units on to a sink T.  The kernels run successive
// shortest paths on the residual graph of that flow, whose arcs are never stored:
//   - partition p led by u = row[lead[p]] gives u -> row[j] for every other slot j: cost -1 when j == 0 (back to the original
//     leader), +1 when lead[p] == 0 (away from it), 0 otherwise.  One lane handles one slot (p, j);
//   - b -> T (cost 0) while f(b) < hi, T -> b (cost 0) while f(b) > lo.  One lane handles one broker.
// Start: lead = 0, f(b) = clamp(leaders(b), lo, hi), excess e(b) = leaders(b) - f(b), e(T) = sum f - P.  No arc is negative yet, so
// this pseudoflow is optimal for its imbalances.  A PHASE:
//   1. keys (distance, arcs on the path) of every node from the nodes with e > 0, by Jacobi relaxation rounds over all arcs until a
//      round changes nothing.  A key is (distance + 2^30) << 32 | arcs, minimised as one 64-bit word: the shortest distance first,
//      the fewest arcs second.  Costs are -1 / 0 / +1 and zero-cost cycles exist, but every cycle adds arcs, so the keys are well
//      defined and the arcs that are tight for them form no cycle.  Round r reads buffer r & 1 and atomicMins into the other one,
//      which holds the keys of round r - 1 (never smaller); every node also bids its own key, so the result is the Jacobi step and
//      "changed" depends on the keys read alone: the round count is a function of the input.
//   2. every tight arc bids its id into pred[head] (32-bit atomicMin): one predecessor per node, the lowest arc id.
//   3. one lane walks the deficit nodes (e < 0) in index order and augments each one's predecessor path when it (a) uses no partition
//      an earlier path of this phase used, (b) keeps every f(b) inside [lo, hi], (c) ends at a node that still has excess.  All
//      those paths consist of arcs that are tight for the phase's keys, so the keys stay feasible potentials for the residual graph
//      after every one of them (a reversed tight arc is tight): no negative cycle appears and the pseudoflow stays optimal for its
//      imbalances.  The first deficit node reached always gets its path, so a phase without a path proves that no deficit node is
//      reachable: the band cannot be met.
// The loop ends with no excess left (the flow is a min-cost flow: OPTIMAL_PROVEN) or with such a phase (INFEASIBLE_PROVEN).
// Two regimes: topics of at most kLeadSoloSlots replica slots and kLeadSoloNodes nodes run the whole solve in ONE workgroup with the
// node state in LDS (k_lead_solo); larger ones launch one kernel per relaxation round over all arcs, the host reading the rounds'
// "changed" flags every kSettleBatch rounds (settle_rounds, kao_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "kao_host.h"
#include "kao_plan_dev.h"   // the 64-bit flow keys, lane_count_to, swap_leader

namespace {

constexpr int kLeadThreads = 256;        // per-round launches
constexpr int kLeadSoloThreads = 1024;   // the persistent workgroup
constexpr int kLeadSoloNodes = 2048;     // B + 1 nodes whose state fits the persistent kernel's LDS (28 bytes per node)
constexpr int kLeadSoloSlots = 1 << 16;  // replica slots up to which one workgroup runs the whole solve
enum { LC_PHASES = 0, LC_ROUNDS = 1, LC_PATHS = 2, LC_MAXLEN = 3, LC_OVER = 4, LC_UNDER = 5, LC_LAUNCHES = 6, LC_LEFT = 7,
       LC_CHANGED = 8, LC_AUG = 9, LC_SUMF = 10, LC_ERR = 11, LC_N = 16 };

// tail, head and cost of the arc of slot s = p * RF + j; false when j is the leader's slot (no arc)
__device__ __forceinline__ bool lead_arc(int s, int RF, const uint16_t *__restrict__ rows, const uint8_t *lead, int &u, int &v, int &c) {
    const int p = s / RF, j = s - p * RF, l = lead[p];
    if (j == l) return false;
    u = rows[p * RF + l];
    v = rows[s];
    c = flow_slot_cost(j, l, true);
    return true;
}

// one Jacobi round, the part of slot s: X is read, Y takes the bids
__device__ __forceinline__ bool lead_relax_slot(int s, int RF, const uint16_t *__restrict__ rows, const uint8_t *lead,
                                                const u64 *X, u64 *Y) {
    int u, v, c;
    if (!lead_arc(s, RF, rows, lead, u, v, c)) return false;
    const u64 ku = X[u];
    if (ku == kFlowInf) return false;
    const u64 nk = flow_step(ku, c);
    if (nk >= X[v]) return false;
    atomicMin(&Y[v], nk);
    return true;
}

// ... the part of node v (v == B: the sink, which only bids its own key)
__device__ __forceinline__ bool lead_relax_node(int v, int B, int lo, int hi, const int32_t *f, const u64 *X,
                                                u64 *Y) {
    const u64 kv = X[v];
    if (kv != kFlowInf) atomicMin(&Y[v], kv);
    if (v == B) return false;
    const u64 kt = X[B];
    bool ch = false;   // (the two bids spelled out: through lc_bid of kao_leaders_cluster.hip the same tests compile to other code here)
    if (f[v] < hi && kv != kFlowInf && kv + 1 < kt) { atomicMin(&Y[B], kv + 1); ch = true; }
    if (f[v] > lo && kt != kFlowInf && kt + 1 < kv) { atomicMin(&Y[v], kt + 1); ch = true; }
    return ch;
}

// predecessor bids: arc ids are s for the partition arcs, PRF + b for b -> T, PRF + B for T -> b
__device__ __forceinline__ void lead_pred_slot(int s, int RF, const uint16_t *__restrict__ rows, const uint8_t *lead,
                                               const u64 *K, uint32_t *pred) {
    int u, v, c;
    if (!lead_arc(s, RF, rows, lead, u, v, c)) return;
    const u64 ku = K[u];
    if (ku != kFlowInf && flow_step(ku, c) == K[v]) atomicMin(&pred[v], (uint32_t)s);
}

__device__ __forceinline__ void lead_pred_node(int b, int B, int PRF, int lo, int hi, const int32_t *f, const u64 *K,
                                               uint32_t *pred) {
    const u64 kb = K[b], kt = K[B];
    if (f[b] < hi && kb != kFlowInf && kb + 1 == kt) atomicMin(&pred[B], (uint32_t)(PRF + b));
    if (f[b] > lo && kt != kFlowInf && kt + 1 == kb) atomicMin(&pred[b], (uint32_t)(PRF + B));
}

// Step 3 of a phase, one lane: returns the paths augmented, *maxlen the longest of them in arcs.
__device__ __forceinline__ int lead_extract(int P, int RF, int B, int lo, int hi, int32_t stamp, const uint16_t *__restrict__ rows,
                                            uint8_t *lead, int32_t *claim, const u64 *K, const uint32_t *pred,
                                            int32_t *e, int32_t *f, int32_t *maxlen) {
    const int PRF = P * RF;
    int naug = 0;
    for (int t = 0; t <= B; ++t) {
        while (e[t] < 0 && K[t] != kFlowInf) {
            bool ok = true;
            int v = t, steps = 0;
            while ((uint32_t)K[v] != 0u) {   // arcs on the way here: 0 at the path's first node
                const uint32_t a = pred[v];
                int u = 0;
                if (a == kFlowNoPred || ++steps > B + 1) { ok = false; break; }   // (a tight path always has its predecessors)
                if (a < (uint32_t)PRF) {
                    const int p = (int)a / RF;
                    if (claim[p] == stamp) { ok = false; break; }
                    u = rows[p * RF + lead[p]];
                } else if (a < (uint32_t)(PRF + B)) {
                    u = (int)a - PRF;
                    if (f[u] >= hi) { ok = false; break; }
                } else {
                    u = B;
                    if (f[v] <= lo) { ok = false; break; }
                }
                v = u;
            }
            if (!ok || e[v] <= 0) break;
            v = t;
            while ((uint32_t)K[v] != 0u) {
                const uint32_t a = pred[v];
                int u;
                if (a < (uint32_t)PRF) {
                    const int p = (int)a / RF;
                    u = rows[p * RF + lead[p]];
                    lead[p] = (uint8_t)((int)a - p * RF);
                    claim[p] = stamp;
                } else if (a < (uint32_t)(PRF + B)) {
                    u = (int)a - PRF;
                    f[u] += 1;
                } else {
                    u = B;
                    f[v] -= 1;
                }
                v = u;
            }
            e[v] -= 1;
            e[t] += 1;
            ++naug;
            *maxlen = max(*maxlen, (int32_t)(uint32_t)K[t]);
        }
    }
    return naug;
}

// the output rows: slot 0 and the chosen leader's slot swapped; returns whether p changed
__device__ __forceinline__ bool lead_swap(int p, int RF, uint16_t *rows, const uint8_t *lead) {
    const int l = lead[p];
    if (l == 0) return false;
    swap_leader(rows + p * RF, l);
    return true;
}

// ---- the whole solve in one workgroup, node state in LDS --------------------------------------------------------------------------
__global__ __launch_bounds__(kLeadSoloThreads) void k_lead_solo(int P, int RF, int B, int lo, int hi, uint16_t *__restrict__ rows,
                                                                uint8_t *__restrict__ lead, int32_t *__restrict__ claim,
                                                                int32_t *__restrict__ ctl) {
    __shared__ u64 key0[kLeadSoloNodes], key1[kLeadSoloNodes];
    __shared__ uint32_t pred[kLeadSoloNodes];
    __shared__ int32_t e[kLeadSoloNodes], f[kLeadSoloNodes];
    __shared__ int32_t sh[LC_N];
    const int tid = threadIdx.x, NT = blockDim.x, N = B + 1, PRF = P * RF;
    for (int v = tid; v < N; v += NT) { e[v] = 0; f[v] = 0; }
    if (tid < LC_N) sh[tid] = 0;
    __syncthreads();
    for (int p = tid; p < P; p += NT) {
        lead[p] = 0;
        claim[p] = 0;
        atomicAdd(&e[rows[p * RF]], 1);
    }
    __syncthreads();
    for (int b = tid; b < B; b += NT) {
        const int c = e[b], fb = min(max(c, lo), hi);
        f[b] = fb;
        e[b] = c - fb;
        if (c > hi) atomicAdd(&sh[LC_OVER], c - hi);
        if (c < lo) atomicAdd(&sh[LC_UNDER], lo - c);
        atomicAdd(&sh[LC_SUMF], fb);
    }
    __syncthreads();
    if (tid == 0) {
        e[B] = sh[LC_SUMF] - P;
        sh[LC_LEFT] = sh[LC_OVER] + max(e[B], 0);
    }
    __syncthreads();
    int phases = 0, rounds = 0, paths = 0;
    while (sh[LC_LEFT] > 0) {
        ++phases;
        for (int v = tid; v < N; v += NT) flow_seed(v, e, key0, key1, pred);
        __syncthreads();
        for (int r = 0;; ++r) {
            if (tid == 0) sh[LC_AUG] = 0;
            __syncthreads();
            const u64 *X = (r & 1) ? key1 : key0;
            u64 *Y = (r & 1) ? key0 : key1;
            bool ch = false;
            for (int s = tid; s < PRF; s += NT) ch |= lead_relax_slot(s, RF, rows, lead, X, Y);
            for (int v = tid; v < N; v += NT) ch |= lead_relax_node(v, B, lo, hi, f, X, Y);
            if (ch) sh[LC_AUG] = 1;
            __syncthreads();
            ++rounds;
            const bool any = sh[LC_AUG] != 0;
            __syncthreads();
            if (!any) break;
            if (r > N) {   // cannot happen (no negative cycle: keys settle within N rounds); the host stops on it
                if (tid == 0) sh[LC_ERR] = 1;
                break;
            }
        }
        __syncthreads();
        if (sh[LC_ERR]) break;
        for (int s = tid; s < PRF; s += NT) lead_pred_slot(s, RF, rows, lead, key0, pred);
        for (int b = tid; b < B; b += NT) lead_pred_node(b, B, PRF, lo, hi, f, key0, pred);
        __syncthreads();
        if (tid == 0) {
            const int n = lead_extract(P, RF, B, lo, hi, phases, rows, lead, claim, key0, pred, e, f, &sh[LC_MAXLEN]);
            sh[LC_AUG] = n;
            sh[LC_LEFT] -= n;
        }
        __syncthreads();
        const int n = sh[LC_AUG];
        paths += n;
        __syncthreads();
        if (n == 0) break;
    }
    if (sh[LC_LEFT] == 0 && !sh[LC_ERR]) {
        int cnt = 0;
        for (int p = tid; p < P; p += NT) cnt += lead_swap(p, RF, rows, lead) ? 1 : 0;
        if (cnt) atomicAdd(&sh[LC_CHANGED], cnt);
    }
    __syncthreads();
    if (tid == 0) {
        sh[LC_PHASES] = phases;
        sh[LC_ROUNDS] = rounds;
        sh[LC_PATHS] = paths;
    }
    __syncthreads();
    if (tid < LC_N) ctl[tid] = sh[tid];
}

// ---- one launch per step, node state in HBM ---------------------------------------------------------------------------------------
__global__ void k_lead_count(int P, int RF, const uint16_t *__restrict__ rows, uint8_t *__restrict__ lead, int32_t *__restrict__ claim,
                             int32_t *__restrict__ e) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    lead[p] = 0;
    claim[p] = 0;
    atomicAdd(&e[rows[(size_t)p * RF]], 1);
}

// e[b] holds leaders(b) on entry; e[B] and ctl are zero
__global__ void k_lead_start(int P, int B, int lo, int hi, int32_t *__restrict__ e, int32_t *__restrict__ f, int32_t *__restrict__ ctl) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int c = e[b], fb = min(max(c, lo), hi);
    f[b] = fb;
    e[b] = c - fb;
    if (c > hi) atomicAdd(&ctl[LC_OVER], c - hi);
    if (c < lo) atomicAdd(&ctl[LC_UNDER], lo - c);
    atomicAdd(&e[B], b == 0 ? fb - P : fb);
}

__global__ void k_lead_seed(int B, const int32_t *__restrict__ e, u64 *__restrict__ k0, u64 *__restrict__ k1,
                            uint32_t *__restrict__ pred, int32_t *__restrict__ flags) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < kSettleBatch) flags[v] = 0;
    if (v <= B) flow_seed(v, e, k0, k1, pred);
}

// round r of a batch: thread i handles slot i and node i; flags[slot of the round in its batch] = 1 when the round changed a key
__global__ void k_lead_round(int r, int P, int RF, int B, int lo, int hi, const uint16_t *__restrict__ rows, const uint8_t *__restrict__ lead,
                             const int32_t *__restrict__ f, u64 *__restrict__ k0, u64 *__restrict__ k1,
                             int32_t *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 *X = (r & 1) ? k1 : k0;
    u64 *Y = (r & 1) ? k0 : k1;
    bool ch = false;
    if (i < P * RF) ch |= lead_relax_slot(i, RF, rows, lead, X, Y);
    if (i <= B) ch |= lead_relax_node(i, B, lo, hi, f, X, Y);
    if (__any(ch) && __lane_id() == 0) *flag = 1;
}

__global__ void k_lead_pred(int P, int RF, int B, int lo, int hi, const uint16_t *__restrict__ rows, const uint8_t *__restrict__ lead,
                            const int32_t *__restrict__ f, const u64 *__restrict__ K, uint32_t *__restrict__ pred) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P * RF) lead_pred_slot(i, RF, rows, lead, K, pred);
    if (i < B) lead_pred_node(i, B, P * RF, lo, hi, f, K, pred);
}

__global__ void k_lead_extract(int P, int RF, int B, int lo, int hi, int32_t stamp, const uint16_t *__restrict__ rows, uint8_t *__restrict__ lead,
                               int32_t *__restrict__ claim, const u64 *__restrict__ K, const uint32_t *__restrict__ pred,
                               int32_t *__restrict__ e, int32_t *__restrict__ f, int32_t *__restrict__ ctl) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int32_t maxlen = ctl[LC_MAXLEN];
    const int n = lead_extract(P, RF, B, lo, hi, stamp, rows, lead, claim, K, pred, e, f, &maxlen);
    ctl[LC_MAXLEN] = maxlen;
    ctl[LC_AUG] = n;
    ctl[LC_PATHS] += n;
}

__global__ void k_lead_apply(int P, int RF, uint16_t *__restrict__ rows, const uint8_t *__restrict__ lead, int32_t *__restrict__ ctl) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    lane_count_to(p < P && lead_swap(p, RF, rows, lead), &ctl[LC_CHANGED]);
}

// keeps its own row loop: complete rows only, under messages of its own (the other planners: check_rows, kao_host.h)
int validate_leaders(const kao_topic *t, const uint16_t *a, const int32_t *n_changed, const int32_t *status, int32_t bd[8]) {
    if (!t || !a || !n_changed || !status) return fail(KAO_ERR_INVALID, "kao_balance_leaders: null pointer");
    int rc = validate(t);   // also the limits: rf <= KAO_MAX_RF, n_brokers <= 65534, P * rf <= 4,000,000 (KAO_ERR_UNSUPPORTED)
    if (rc) return rc;
    derive_bounds(t, bd);
    if (bd[2] > bd[3]) return fail(KAO_ERR_INVALID, "kao_balance_leaders: lead_lo > lead_hi");
    const int RF = t->rf;
    for (int64_t p = 0; p < t->n_partitions; ++p) {
        const uint16_t *row = a + p * RF;
        for (int i = 0; i < RF; ++i) {
            if (row[i] >= t->n_brokers)
                return fail(KAO_ERR_INVALID, "kao_balance_leaders: partition " + std::to_string(p) + ": slot " + std::to_string(i) +
                                                 " holds no broker of the topic (complete rows only)");
            for (int j = 0; j < i; ++j)
                if (row[j] == row[i]) return fail(KAO_ERR_INVALID, "kao_balance_leaders: partition " + std::to_string(p) + ": broker repeated in a row");
        }
    }
    return KAO_OK;
}

}  // namespace

extern "C" int kao_balance_leaders(const kao_topic *t, uint16_t *assignment, int32_t *n_changed, int64_t *objective, int32_t *status,
                                   int32_t stats[8]) {
    int32_t bd[8];
    int rc = validate_leaders(t, assignment, n_changed, status, bd);
    if (rc) return rc;
    if ((rc = require_init())) return rc;
    const int P = t->n_partitions, RF = t->rf, B = t->n_brokers, N = B + 1, PRF = P * RF, lo = bd[2], hi = bd[3];
    const bool solo = N <= kLeadSoloNodes && PRF <= kLeadSoloSlots;

    // one arena: rows u16[PRF] | lead u8[P] | claim i32[P] | ctl i32[LC_N] | flags i32[kSettleBatch] | e, f i32[N] | pred u32[N] | keys u64[2][N]
    Carve cv;
    const size_t o_rows = cv.take<uint16_t>(PRF), o_lead = cv.take<uint8_t>(P), o_claim = cv.take<int32_t>(P), o_ctl = cv.take<int32_t>(LC_N),
                 o_flags = cv.take<int32_t>(kSettleBatch), o_e = cv.take<int32_t>(N), o_f = cv.take<int32_t>(N), o_pred = cv.take<uint32_t>(N),
                 o_k0 = cv.take<u64>(N), o_k1 = cv.take<u64>(N);
    CallBufs m;
    if ((rc = m.open(cv.end()))) return rc;
    hipStream_t st = m.stream;
    uint16_t *d_rows = m.at<uint16_t>(o_rows);
    uint8_t *d_lead = m.at<uint8_t>(o_lead);
    int32_t *d_claim = m.at<int32_t>(o_claim), *d_ctl = m.at<int32_t>(o_ctl), *d_flags = m.at<int32_t>(o_flags), *d_e = m.at<int32_t>(o_e),
            *d_f = m.at<int32_t>(o_f);
    uint32_t *d_pred = m.at<uint32_t>(o_pred);
    u64 *d_k0 = m.at<u64>(o_k0), *d_k1 = m.at<u64>(o_k1);

    HIP_TRY(hipMemcpyAsync(d_rows, assignment, (size_t)PRF * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    int32_t ctl[LC_N] = {0};
    int32_t launches = 0;
    if (solo) {
        k_lead_solo<<<1, kLeadSoloThreads, 0, st>>>(P, RF, B, lo, hi, d_rows, d_lead, d_claim, d_ctl);
        HIP_TRY(hipGetLastError());
        launches = 1;
        HIP_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ctl[LC_ERR]) return fail(KAO_ERR_HIP, "kao_balance_leaders: relaxation did not settle");
    } else {
        const unsigned pblocks = grid_for(P, kLeadThreads), nblocks = grid_for(N, kLeadThreads), ablocks = grid_for(std::max(PRF, N), kLeadThreads);
        HIP_TRY(hipMemsetAsync(d_ctl, 0, o_f - o_ctl, st));   // ctl, flags, e
        k_lead_count<<<pblocks, kLeadThreads, 0, st>>>(P, RF, d_rows, d_lead, d_claim, d_e);
        k_lead_start<<<nblocks, kLeadThreads, 0, st>>>(P, B, lo, hi, d_e, d_f, d_ctl);
        HIP_TRY(hipGetLastError());
        launches = 2;
        int32_t e_sink = 0;
        HIP_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&e_sink, d_e + B, sizeof e_sink, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int32_t phases = 0, rounds = 0, left = ctl[LC_OVER] + std::max(e_sink, 0);
        while (left > 0) {   // a phase per turn
            ++phases;
            k_lead_seed<<<nblocks, kLeadThreads, 0, st>>>(B, d_e, d_k0, d_k1, d_pred, d_flags);
            ++launches;
            if ((rc = settle_rounds("kao_balance_leaders: ", st, N, d_flags, rounds, launches, [&](int r, int32_t *flag) {
                    k_lead_round<<<ablocks, kLeadThreads, 0, st>>>(r, P, RF, B, lo, hi, d_rows, d_lead, d_f, d_k0, d_k1, flag);
                })))
                return rc;
            k_lead_pred<<<ablocks, kLeadThreads, 0, st>>>(P, RF, B, lo, hi, d_rows, d_lead, d_f, d_k0, d_pred);
            k_lead_extract<<<1, 64, 0, st>>>(P, RF, B, lo, hi, phases, d_rows, d_lead, d_claim, d_k0, d_pred, d_e, d_f, d_ctl);
            launches += 2;
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            left -= ctl[LC_AUG];
            if (ctl[LC_AUG] == 0) break;
        }
        if (left == 0) {
            k_lead_apply<<<pblocks, kLeadThreads, 0, st>>>(P, RF, d_rows, d_lead, d_ctl);
            HIP_TRY(hipGetLastError());
            ++launches;
            HIP_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        ctl[LC_PHASES] = phases;
        ctl[LC_ROUNDS] = rounds;
        ctl[LC_LEFT] = left;
    }
    const bool feasible = ctl[LC_LEFT] == 0;
    if (feasible) {
        HIP_TRY(hipMemcpyAsync(assignment, d_rows, (size_t)PRF * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_changed = feasible ? ctl[LC_CHANGED] : 0;
    *status = feasible ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_INFEASIBLE_PROVEN;
    if (stats) {
        for (int i = 0; i < 6; ++i) stats[i] = ctl[i];
        stats[6] = launches;
        stats[7] = ctl[LC_LEFT];
    }
    if (objective) {
        int32_t viol[8];
        if ((rc = kao_evaluate(t, assignment, objective, viol))) return rc;
    }
    return KAO_OK;
}
