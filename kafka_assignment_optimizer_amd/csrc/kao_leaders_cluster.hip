// kao_leaders_cluster.hip -- kao_balance_leaders_cluster: the preferred leaders of all topics chosen together, replica sets kept, so
// that every topic's leader band holds, every broker leads at least cluster_lo partitions, the largest cluster-wide leader count is as
// low as it can be and the fewest leaders change.  Kernels and the C entry point.
//
// For a cap M this is a min-cost flow on partition -> (topic, broker) -> broker -> sink: partition p sends one unit to the pair node of
// the slot it picks as leader (cost 0 for slot 0, 1 otherwise), pair q = (t, b) passes g(q) in [topic_lo[t], topic_hi[t]] on to broker
// b, broker b passes f(b) in [cluster_lo, M] on to the sink T.  Nodes: the Q occurring pairs, then the B brokers, then T.  The residual
// arcs are never stored:
//   - partition p led by slot l gives pair(p, l) -> pair(p, j) for every other non-empty slot j: cost -1 when j == 0, +1 when l == 0,
//     0 otherwise (all 0 in a probe).  One lane per slot; arc id p * W + j;
//   - pair q -> its broker while g(q) < hi(q) (id PW + q), broker -> q while g(q) > lo(q) (id PW + Q + q).  One lane per pair;
//   - broker b -> T while f(b) < M (id PW + 2Q + b), T -> b while f(b) > cluster_lo (id PW + 2Q + B + b).  One lane per broker.
// A SOLVE at cap M starts from j = 0 with the pseudoflow clamped into its bounds on both levels: g = clamp(leaders(q)), e(q) =
// leaders(q) - g, f = clamp(sum of g over the pairs of b), e(b) = that sum - f, e(T) = sum f - P.  No residual arc is negative there.
// Its PHASES are those of kao_leaders.hip, on the flow keys of kao_plan_dev.h: (1) keys (distance + 2^30) << 32 | arcs of every node
// from the nodes with e > 0, Jacobi rounds between two buffers until a round changes nothing; (2) every tight arc bids its id into pred[head], the lowest id wins;
// the nodes below T with e < 0 and a key are marked, and when T has e < 0 so are the brokers with room whose distance equals T's
// (their arcs into T have reduced cost 0); (3) one lane serves the marked nodes in index order, then the marked brokers in index
// order, and augments a node's predecessor path while it uses no partition an earlier path of the phase used, keeps every g and f
// inside its bounds and ends at a node that still has excess.  All those paths consist of arcs of reduced cost 0 for the phase's
// distances, so the distances stay feasible potentials and the pseudoflow stays optimal for its imbalances.  The first marked node
// always gets its path: a phase without a path proves the cap infeasible.
// M is never raised inside a running solve (section 4i's warning): with cluster_hi = -1 one probe without a cap decides
// INFEASIBLE_PROVEN, the cap is bisected over probes (max-flows: all costs 0) between max(ceil(P / B), cluster_lo) and the peak of the
// last feasible probe, and one min-cost solve runs at the optimum; every one of them starts over from j = 0.
// Node state lives in HBM / L2 (config 4 has 28,038 pair nodes): one launch per relaxation round, the host reading the rounds'
// "changed" flags every kSettleBatch rounds (settle_rounds, kao_host.h) and the counters after every phase.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "kao_host.h"
#include "kao_plan_dev.h"   // the 64-bit flow keys, lane_count_to, swap_leader

namespace {

constexpr int kLcThreads = 256;
enum { CC_PATHS = 0, CC_MAXLEN = 1, CC_AUG = 2, CC_OVER = 3, CC_PEAK0 = 4, CC_PEAK = 5, CC_CHANGED = 6, CC_N = 8 };

struct LcNet {   // the network of one call; every pointer is device memory
    int P, W, B, Q, N, PW;
    const uint16_t *rows;       // [PW]
    const int32_t *pair_of;     // [PW] pair node of a slot, -1 for an empty one
    const int32_t *bro;         // [Q] broker of a pair
    const int32_t *plo, *phi;   // [Q] band of a pair's topic
    uint8_t *lead;              // [P] chosen slot
    int32_t *claim;             // [P] phase stamp of the last path through p
    int32_t *c0;                // [Q] leaders of a pair at j = 0
    int32_t *g, *f, *inb;       // [Q], [B], [B]
    int32_t *e;                 // [N]
    u64 *k0, *k1;   // [N]
    uint32_t *pred;             // [N]
    uint8_t *mark;              // [N]: bit 0 = a node below T to serve, bit 1 = broker b (at Q + b) is a tight way into T while T is served
    int32_t *ctl;               // [CC_N]
};

// tail, head and cost of the arc of slot s = p * W + j; false when j is the leader's slot or empty
__device__ __forceinline__ bool lc_arc(int s, const LcNet &n, bool costed, int &u, int &v, int &c) {
    v = n.pair_of[s];
    if (v < 0) return false;
    const int p = s / n.W, j = s - p * n.W, l = n.lead[p];
    if (j == l) return false;
    u = n.pair_of[p * n.W + l];
    c = flow_slot_cost(j, l, costed);
    return true;
}

// an arc of cost 0 from a node with key ku to one with key kv bids into the head's word of the other buffer when it lowers the key
__device__ __forceinline__ bool lc_bid(u64 ku, u64 kv, u64 *yv) {
    if (ku == kFlowInf || ku + 1 >= kv) return false;
    atomicMin(yv, ku + 1);
    return true;
}

// ---- once per call ------------------------------------------------------------------------------------------------------------------
__global__ void k_lc_count(LcNet n, int32_t *__restrict__ cnt0) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n.P) return;
    n.claim[p] = 0;
    atomicAdd(&n.c0[n.pair_of[(size_t)p * n.W]], 1);
    atomicAdd(&cnt0[n.rows[(size_t)p * n.W]], 1);
}

__global__ void k_lc_max(int B, const int32_t *__restrict__ x, int32_t *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B && x[b] > 0) atomicMax(out, x[b]);
}

// ---- the start of a solve -----------------------------------------------------------------------------------------------------------
// inb, e[T] and ctl[CC_OVER] are zero on entry
__global__ void k_lc_start_pairs(LcNet n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n.P) n.lead[i] = 0;
    if (i >= n.Q) return;
    const int c = n.c0[i], gq = min(max(c, n.plo[i]), n.phi[i]);
    n.g[i] = gq;
    n.e[i] = c - gq;
    if (gq) atomicAdd(&n.inb[n.bro[i]], gq);
    if (c > gq) atomicAdd(&n.ctl[CC_OVER], c - gq);
}

__global__ void k_lc_start_brokers(LcNet n, int clo, int M) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n.B) return;
    const int c = n.inb[b], fb = min(max(c, clo), M);
    n.f[b] = fb;
    n.e[n.Q + b] = c - fb;
    if (c > fb) atomicAdd(&n.ctl[CC_OVER], c - fb);
    atomicAdd(&n.e[n.N - 1], b == 0 ? fb - n.P : fb);
}

// ---- a phase ------------------------------------------------------------------------------------------------------------------------
__global__ void k_lc_seed(LcNet n, int32_t *__restrict__ flags) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < kSettleBatch) flags[v] = 0;
    if (v >= n.N) return;
    flow_seed(v, n.e, n.k0, n.k1, n.pred);
    n.mark[v] = 0;
}

// round r: thread i handles slot i, pair i, broker i and the own bid of node i
__global__ void k_lc_round(LcNet n, int r, int costed, int clo, int M, int32_t *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 *X = (r & 1) ? n.k1 : n.k0;
    u64 *Y = (r & 1) ? n.k0 : n.k1;
    bool ch = false;
    if (i < n.PW) {
        int u, v, c;
        if (lc_arc(i, n, costed != 0, u, v, c)) {
            const u64 ku = X[u];
            if (ku != kFlowInf) {
                const u64 nk = flow_step(ku, c);
                if (nk < X[v]) { atomicMin(&Y[v], nk); ch = true; }
            }
        }
    }
    if (i < n.Q) {
        const int nb = n.Q + n.bro[i], gq = n.g[i];
        const u64 kq = X[i], kb = X[nb];
        if (gq < n.phi[i]) ch |= lc_bid(kq, kb, &Y[nb]);
        if (gq > n.plo[i]) ch |= lc_bid(kb, kq, &Y[i]);
    }
    if (i < n.B) {
        const int nb = n.Q + i, T = n.N - 1, fb = n.f[i];
        const u64 kb = X[nb], kt = X[T];
        if (fb < M) ch |= lc_bid(kb, kt, &Y[T]);
        if (fb > clo) ch |= lc_bid(kt, kb, &Y[nb]);
    }
    if (i < n.N) {
        const u64 kv = X[i];
        if (kv != kFlowInf) atomicMin(&Y[i], kv);
    }
    if (__any(ch) && __lane_id() == 0) *flag = 1;
}

// the settled keys are in both buffers
__global__ void k_lc_pred(LcNet n, int costed, int clo, int M) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 *K = n.k0;
    const int T = n.N - 1;
    if (i < n.PW) {
        int u, v, c;
        if (lc_arc(i, n, costed != 0, u, v, c)) {
            const u64 ku = K[u];
            if (ku != kFlowInf && flow_step(ku, c) == K[v]) atomicMin(&n.pred[v], (uint32_t)i);
        }
    }
    if (i < n.Q) {
        const int nb = n.Q + n.bro[i], gq = n.g[i];
        const u64 kq = K[i], kb = K[nb];
        if (gq < n.phi[i] && kq != kFlowInf && kq + 1 == kb) atomicMin(&n.pred[nb], (uint32_t)(n.PW + i));
        if (gq > n.plo[i] && kb != kFlowInf && kb + 1 == kq) atomicMin(&n.pred[i], (uint32_t)(n.PW + n.Q + i));
        if (n.e[i] < 0 && kq != kFlowInf) n.mark[i] = 1;
    }
    if (i < n.B) {
        const int nb = n.Q + i, fb = n.f[i];
        const u64 kb = K[nb], kt = K[T];
        if (fb < M && kb != kFlowInf && kb + 1 == kt) atomicMin(&n.pred[T], (uint32_t)(n.PW + 2 * n.Q + i));
        if (fb > clo && kt != kFlowInf && kt + 1 == kb) atomicMin(&n.pred[nb], (uint32_t)(n.PW + 2 * n.Q + n.B + i));
        // bit 0: a deficit node to serve; bit 1: a way into T of reduced cost 0, tried when T is served
        uint8_t m = 0;
        if (n.e[nb] < 0 && kb != kFlowInf) m |= 1;
        if (n.e[T] < 0 && kt != kFlowInf && fb < M && kb != kFlowInf && (kb >> 32) == (kt >> 32)) m |= 2;
        n.mark[nb] = m;
    }
}

// (the walk differs from lead_extract of kao_leaders.hip in its arc classes and its two passes: not shared)
// One lane: the predecessor path of node v0 back to its first node.  apply = false checks it against the paths this phase has
// already taken (returns -1 when it is blocked), apply = true takes it.  Returns the first node.
__device__ int lc_walk(const LcNet &n, int v0, int32_t stamp, int clo, int M, bool apply) {
    const int T = n.N - 1, a_up = n.PW, a_dn = n.PW + n.Q, a_bt = n.PW + 2 * n.Q, a_tb = a_bt + n.B;
    int v = v0, steps = 0;
    while ((uint32_t)n.k0[v] != 0u) {   // arcs on the way here: 0 at the path's first node
        const uint32_t a = n.pred[v];
        int u;
        if (a == kFlowNoPred || ++steps > n.N) return -1;   // (a tight path always has its predecessors)
        if (a < (uint32_t)a_up) {
            const int p = (int)a / n.W;
            if (!apply && n.claim[p] == stamp) return -1;
            u = n.pair_of[p * n.W + n.lead[p]];
            if (apply) { n.lead[p] = (uint8_t)((int)a - p * n.W); n.claim[p] = stamp; }
        } else if (a < (uint32_t)a_dn) {
            u = (int)a - a_up;
            if (!apply && n.g[u] >= n.phi[u]) return -1;
            if (apply) n.g[u] += 1;
        } else if (a < (uint32_t)a_bt) {
            const int q = (int)a - a_dn;
            u = n.Q + n.bro[q];
            if (!apply && n.g[q] <= n.plo[q]) return -1;
            if (apply) n.g[q] -= 1;
        } else if (a < (uint32_t)a_tb) {
            const int b = (int)a - a_bt;
            u = n.Q + b;
            if (!apply && n.f[b] >= M) return -1;
            if (apply) n.f[b] += 1;
        } else {
            const int b = (int)a - a_tb;
            u = T;
            if (!apply && n.f[b] <= clo) return -1;
            if (apply) n.f[b] -= 1;
        }
        v = u;
    }
    return v;
}

// Step 3 of a phase.  One wavefront: all lanes look for marked nodes, 64 at a time; lane 0 serves them.  The marks are those of the
// phase's start (k_lc_pred), so the nodes tried and their order depend on the input alone.
__global__ __launch_bounds__(64) void k_lc_extract(LcNet n, int32_t stamp, int clo, int M) {
    const int lane = threadIdx.x, T = n.N - 1;
    int naug = 0, maxlen = 0;
    for (int base = 0; base < T; base += 64) {
        const int v = base + lane;
        u64 m = __ballot(v < T && (n.mark[v] & 1));
        while (lane == 0 && m) {
            const int t = base + __ffsll((long long)m) - 1;
            m &= m - 1;
            while (n.e[t] < 0) {
                const int src = lc_walk(n, t, stamp, clo, M, false);
                if (src < 0 || n.e[src] <= 0) break;
                lc_walk(n, t, stamp, clo, M, true);
                n.e[src] -= 1;
                n.e[t] += 1;
                ++naug;
                maxlen = max(maxlen, (int)(uint32_t)n.k0[t]);
            }
        }
    }
    for (int base = 0; base < n.B; base += 64) {
        const int b = base + lane;
        u64 m = __ballot(b < n.B && (n.mark[n.Q + b] & 2));
        while (lane == 0 && m) {
            const int t = base + __ffsll((long long)m) - 1;
            m &= m - 1;
            while (n.e[T] < 0 && n.f[t] < M) {
                const int src = lc_walk(n, n.Q + t, stamp, clo, M, false);
                if (src < 0 || n.e[src] <= 0) break;
                lc_walk(n, n.Q + t, stamp, clo, M, true);
                n.f[t] += 1;
                n.e[src] -= 1;
                n.e[T] += 1;
                ++naug;
                maxlen = max(maxlen, (int)(uint32_t)n.k0[n.Q + t] + 1);
            }
        }
    }
    if (lane == 0) {
        n.ctl[CC_AUG] = naug;
        n.ctl[CC_PATHS] += naug;
        n.ctl[CC_MAXLEN] = max(n.ctl[CC_MAXLEN], maxlen);
    }
}

// ---- the result ---------------------------------------------------------------------------------------------------------------------
__global__ void k_lc_apply(LcNet n, uint16_t *__restrict__ rows, int dry_run) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool ch = false;
    if (p < n.P) {
        const int l = n.lead[p];
        ch = l != 0;
        if (ch && !dry_run) swap_leader(rows + (size_t)p * n.W, l);
    }
    lane_count_to(ch, &n.ctl[CC_CHANGED]);
}

int validate_cluster(int32_t B, int32_t P, int32_t W, const uint16_t *rows, const int32_t *topic_of, int32_t T, const int32_t *tlo,
                     const int32_t *thi, int32_t clo, int32_t chi, const int32_t *n_changed, const int32_t *peak_before,
                     const int32_t *peak_after, const int32_t *status) {
    const std::string fn = "kao_balance_leaders_cluster: ";
    if (!rows || !topic_of || !tlo || !thi || !n_changed || !peak_before || !peak_after || !status) return fail(KAO_ERR_INVALID, fn + "null pointer");
    int rc = check_dims(fn, B, P, W);
    if (rc) return rc;
    if (T < 1) return fail(KAO_ERR_INVALID, fn + "n_topics < 1");
    if (clo < 0) return fail(KAO_ERR_INVALID, fn + "cluster_lo < 0");
    if (chi < -1) return fail(KAO_ERR_INVALID, fn + "cluster_hi < -1");
    if (chi >= 0 && chi < clo) return fail(KAO_ERR_INVALID, fn + "cluster_hi < cluster_lo");
    if ((rc = check_slot_cap(fn, P, W))) return rc;
    for (int t = 0; t < T; ++t)
        if (tlo[t] < 0 || tlo[t] > thi[t]) return fail(KAO_ERR_INVALID, fn + "topic " + std::to_string(t) + ": band needs 0 <= topic_lo <= topic_hi");
    for (int64_t p = 0; p < P; ++p) {   // (check_rows, with the row's topic checked in front of it)
        if (topic_of[p] < 0 || topic_of[p] >= T) return fail(KAO_ERR_INVALID, fn + "partition " + std::to_string(p) + ": topic_of outside 0..n_topics-1");
        if ((rc = check_row(fn, B, W, p, rows + p * W))) return rc;
    }
    return KAO_OK;
}

}  // namespace

extern "C" int kao_balance_leaders_cluster(int32_t n_brokers, int32_t n_partitions, int32_t width, uint16_t *rows, const int32_t *topic_of,
                                           int32_t n_topics, const int32_t *topic_lo, const int32_t *topic_hi, int32_t cluster_lo,
                                           int32_t cluster_hi, int32_t dry_run, int32_t *n_changed, int32_t *peak_before,
                                           int32_t *peak_after, int32_t *status, int32_t stats[8]) {
    int rc = validate_cluster(n_brokers, n_partitions, width, rows, topic_of, n_topics, topic_lo, topic_hi, cluster_lo, cluster_hi, n_changed,
                              peak_before, peak_after, status);
    if (rc) return rc;
    if ((rc = require_init())) return rc;
    const int B = n_brokers, P = n_partitions, W = width, PW = P * W;

    // the dense index of the occurring (topic, broker) pairs, ordered by (topic, broker)
    std::vector<uint64_t> keys;
    keys.reserve((size_t)PW);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < W && rows[(size_t)p * W + j] != KAO_NONE; ++j) keys.push_back((uint64_t)topic_of[p] * (uint64_t)B + rows[(size_t)p * W + j]);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const int Q = (int)keys.size(), N = Q + B + 1;
    std::vector<int32_t> h_pair((size_t)std::max(PW, 1), -1), h_bro((size_t)std::max(Q, 1)), h_plo((size_t)std::max(Q, 1)), h_phi((size_t)std::max(Q, 1));
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < W && rows[(size_t)p * W + j] != KAO_NONE; ++j)
            h_pair[(size_t)p * W + j] =
                (int32_t)(std::lower_bound(keys.begin(), keys.end(), (uint64_t)topic_of[p] * (uint64_t)B + rows[(size_t)p * W + j]) - keys.begin());
    std::vector<int32_t> held((size_t)n_topics, 0);
    for (int q = 0; q < Q; ++q) {
        const int t = (int)(keys[(size_t)q] / (uint64_t)B);
        h_bro[(size_t)q] = (int32_t)(keys[(size_t)q] % (uint64_t)B);
        h_plo[(size_t)q] = topic_lo[t];
        h_phi[(size_t)q] = topic_hi[t];
        ++held[(size_t)t];
    }
    bool possible = true;   // a broker that holds no replica of t leads none of it: topic_lo[t] > 0 cannot be met there
    for (int t = 0; t < n_topics; ++t) possible = possible && (topic_lo[t] == 0 || held[(size_t)t] == B);

    // one arena: ctl i32[CC_N] | flags i32[kSettleBatch] | cnt0 i32[B] | c0 i32[Q] (zeroed once up to here) | inb i32[B] | e i32[N] (zeroed
    //            per solve) | g i32[Q] | f i32[B] | pred u32[N] | k0, k1 u64[N] | pair_of i32[PW] | bro, plo, phi i32[Q] | claim i32[P] |
    //            rows u16[PW] | lead u8[P] | mark u8[N]
    Carve cv;
    const size_t o_ctl = cv.take<int32_t>(CC_N), o_flags = cv.take<int32_t>(kSettleBatch), o_cnt0 = cv.take<int32_t>(B), o_c0 = cv.take<int32_t>(Q),
                 zeroed_once = cv.end(), o_inb = cv.take<int32_t>(B), o_e = cv.take<int32_t>(N), per_solve = cv.end() - o_inb,
                 o_g = cv.take<int32_t>(Q), o_f = cv.take<int32_t>(B), o_pred = cv.take<uint32_t>(N), o_k0 = cv.take<u64>(N), o_k1 = cv.take<u64>(N),
                 o_pair = cv.take<int32_t>(PW), o_bro = cv.take<int32_t>(Q), o_plo = cv.take<int32_t>(Q), o_phi = cv.take<int32_t>(Q),
                 o_claim = cv.take<int32_t>(P), o_rows = cv.take<uint16_t>(PW), o_lead = cv.take<uint8_t>(P), o_mark = cv.take<uint8_t>(N);
    CallBufs m;
    if ((rc = m.open(cv.end()))) return rc;
    hipStream_t st = m.stream;
    uint16_t *d_rows = m.at<uint16_t>(o_rows);
    int32_t *d_flags = m.at<int32_t>(o_flags), *d_cnt0 = m.at<int32_t>(o_cnt0);
    LcNet n;
    n.P = P; n.W = W; n.B = B; n.Q = Q; n.N = N; n.PW = PW;
    n.rows = d_rows; n.pair_of = m.at<int32_t>(o_pair); n.bro = m.at<int32_t>(o_bro); n.plo = m.at<int32_t>(o_plo); n.phi = m.at<int32_t>(o_phi);
    n.lead = m.at<uint8_t>(o_lead); n.claim = m.at<int32_t>(o_claim); n.c0 = m.at<int32_t>(o_c0); n.g = m.at<int32_t>(o_g); n.f = m.at<int32_t>(o_f);
    n.inb = m.at<int32_t>(o_inb); n.e = m.at<int32_t>(o_e); n.k0 = m.at<u64>(o_k0); n.k1 = m.at<u64>(o_k1);
    n.pred = m.at<uint32_t>(o_pred); n.mark = m.at<uint8_t>(o_mark); n.ctl = m.at<int32_t>(o_ctl);

    HIP_TRY(hipMemsetAsync(m.arena, 0, zeroed_once, st));
    if (PW) {
        HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<int32_t>(o_pair), h_pair.data(), (size_t)PW * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    if (Q) {
        HIP_TRY(hipMemcpyAsync(m.at<int32_t>(o_bro), h_bro.data(), (size_t)Q * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<int32_t>(o_plo), h_plo.data(), (size_t)Q * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<int32_t>(o_phi), h_phi.data(), (size_t)Q * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    const unsigned pblocks = grid_for(P, kLcThreads), bblocks = grid_for(B, kLcThreads), nblocks = grid_for(N, kLcThreads),
                   ablocks = grid_for(std::max(PW, N), kLcThreads), sblocks = grid_for(std::max(P, Q), kLcThreads);
    int32_t launches = 0, ctl[CC_N] = {0};
    if (P) {
        k_lc_count<<<pblocks, kLcThreads, 0, st>>>(n, d_cnt0);
        ++launches;
    }
    k_lc_max<<<bblocks, kLcThreads, 0, st>>>(B, d_cnt0, n.ctl + CC_PEAK0);
    ++launches;
    HIP_TRY(hipGetLastError());

    int32_t probes = 0, phases = 0, rounds = 0, left = 0;
    // one solve at cap M from j = 0; *feasible, and ctl[CC_PEAK] = the largest f when it is
    auto solve = [&](int M, bool costed, bool *feasible) -> int {
        ++probes;
        HIP_TRY(hipMemsetAsync(n.inb, 0, per_solve, st));   // inb, e
        HIP_TRY(hipMemsetAsync(n.ctl + CC_OVER, 0, 4, st));
        k_lc_start_pairs<<<sblocks, kLcThreads, 0, st>>>(n);
        k_lc_start_brokers<<<bblocks, kLcThreads, 0, st>>>(n, cluster_lo, M);
        launches += 2;
        HIP_TRY(hipGetLastError());
        int32_t e_sink = 0;
        HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&e_sink, n.e + (N - 1), sizeof e_sink, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        left = ctl[CC_OVER] + std::max(e_sink, 0);
        while (left > 0) {   // a phase per turn
            ++phases;
            k_lc_seed<<<nblocks, kLcThreads, 0, st>>>(n, d_flags);
            ++launches;
            if ((rc = settle_rounds("kao_balance_leaders_cluster: ", st, N, d_flags, rounds, launches, [&](int r, int32_t *flag) {
                    k_lc_round<<<ablocks, kLcThreads, 0, st>>>(n, r, costed ? 1 : 0, cluster_lo, M, flag);
                })))
                return rc;
            k_lc_pred<<<ablocks, kLcThreads, 0, st>>>(n, costed ? 1 : 0, cluster_lo, M);
            k_lc_extract<<<1, 64, 0, st>>>(n, phases, cluster_lo, M);
            launches += 2;
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            left -= ctl[CC_AUG];
            if (ctl[CC_AUG] == 0) break;
        }
        *feasible = left == 0;
        if (*feasible) {
            HIP_TRY(hipMemsetAsync(n.ctl + CC_PEAK, 0, 4, st));
            k_lc_max<<<bblocks, kLcThreads, 0, st>>>(B, n.f, n.ctl + CC_PEAK);
            ++launches;
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return KAO_OK;
    };

    bool feasible = possible;
    if (feasible && cluster_hi >= 0) {
        if ((rc = solve(cluster_hi, true, &feasible))) return rc;
    } else if (feasible) {
        if ((rc = solve(std::max(P, cluster_lo), false, &feasible))) return rc;   // no cap: no broker can lead more than P
        if (feasible) {
            int lo = std::max((P + B - 1) / B, cluster_lo), hi = ctl[CC_PEAK];
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                bool ok = false;
                if ((rc = solve(mid, false, &ok))) return rc;
                if (ok) hi = ctl[CC_PEAK]; else lo = mid + 1;
            }
            if ((rc = solve(hi, true, &feasible))) return rc;
            if (!feasible) return fail(KAO_ERR_HIP, "kao_balance_leaders_cluster: the min-cost solve contradicts its probe");
        }
    }
    if (!possible) {   // peak_before still comes from the device
        HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (feasible && P) {
        k_lc_apply<<<pblocks, kLcThreads, 0, st>>>(n, d_rows, dry_run);
        ++launches;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        if (!dry_run) HIP_TRY(hipMemcpyAsync(rows, d_rows, (size_t)PW * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *peak_before = ctl[CC_PEAK0];
    *peak_after = feasible ? ctl[CC_PEAK] : ctl[CC_PEAK0];
    *n_changed = feasible ? ctl[CC_CHANGED] : 0;
    *status = feasible ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_INFEASIBLE_PROVEN;
    if (stats) {
        stats[0] = probes; stats[1] = phases; stats[2] = rounds; stats[3] = ctl[CC_PATHS]; stats[4] = ctl[CC_MAXLEN]; stats[5] = launches;
        stats[6] = Q; stats[7] = feasible ? 0 : left;
    }
    return KAO_OK;
}
