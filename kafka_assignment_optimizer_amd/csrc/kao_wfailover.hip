// kao_wfailover.hip -- kao_failover_order_weighted: the follower order that keeps the peak TRAFFIC a surviving broker leads after a
// broker or rack failure low.  Kernels and the C entry point.
//
// The scenario model is that of kao_failover_order (section 4i; its classify / offsets / scatter kernels are shared through
// kao_failover_dev.h): scenario g takes down D_g, the partitions led from D_g with a surviving follower are AFFECTED, e(p) is the slot
// Kafka would elect, a choice gives each of them an eligible slot j(p), and swapping e(p) with j(p) moves no data.  Here partition p
// carries weight[p]: Wlead(b) = the weight b leads by preference, L_g(b) = Wlead(b) + the weight b inherits in g.  Minimising
// max L_g is restricted-assignment makespan with fixed base loads (NP-hard), so each scenario runs the deterministic descent of
// section 4k on L_g, with a lower bound computed beside it.
//   k_wfo_wlead   Wlead[] in u64
//   k_wfo_solve   ONE WORKGROUP PER SCENARIO, all scenarios in one launch: every round, then the certificate, then the swaps
// A ROUND uses the loads as they stand at its start and has three parts with a barrier after each:
//   PROPOSE  every affected p with weight > 0 and two eligible slots or more takes b* = its eligible broker other than the current
//            one a with the lowest load (ties: the lowest slot) and proposes a -> b* iff L(b*) + weight + min_gain < L(a); it bids
//            key(p) = (0xFFFF - code(L(a))) << 48 | (0xFFFF - code(weight)) << 32 | p into the ONE minkey word of a and of b* (LDS
//            atomicMin, skipped when the word is already lower).  The barrier is __syncthreads_or("I proposed"): the end test.
//   DECIDE   a proposal wins iff both words hold its key; only minkey words are read, only the partition's own flag is written.
//   APPLY    winners store L(a) -= w, L(b*) += w (no two winners share a broker), every proposer clears its two words.
// No lane reads a load in the part in which another lane can write it: the snapshot rule of section 4k with one minkey row.
// LDS: the u64 load and the u64 minkey word per broker, 16 bytes, 128,000 bytes at KAO_FAILOVER_MAX_BROKERS.
// The CERTIFICATE, valid for any choice of slots, after the last round: T = the surviving brokers eligible for an affected partition,
// compacted (its size is at most the scenario's eligible slots, whatever B is), ranked by final load descending (ties: index
// ascending) by all pairs; the minkey area then maps broker -> rank and the load area becomes the u64 histogram over ranks:
// A_k = the Wlead of the k highest-ranked brokers + the weight of the partitions whose eligible brokers all rank below k.  The bound
// is the maximum of: the survivors' largest Wlead; weight[p] + the smallest Wlead among p's eligible brokers; Wlead(b) + the weight
// of the partitions whose only eligible broker is b; ceil(A_k / k).  Integers only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kao_failover_dev.h"
#include "kao_plan_dev.h"   // DESCENT_KEY, descent_gains, descent_bid

namespace {

constexpr u64 kWfNoKey = ~0ull;
constexpr int kWfHardRounds = 1 << 26;   // no descent gets here; a guard against an endless loop
constexpr int kWfWon = 0x80;             // flag in slot[p]: this round's proposal of p won
enum { WC_SCEN = 0, WC_ROUNDS, WC_MOVES, WC_PROPS, WC_MORE, WC_PROVEN, WC_MAXROUNDS, WC_REORDERED, WC_ERR, WC_N = 16 };
enum { WS_MAXLEAD = 0, WS_PEAK0, WS_PEAK1, WS_MINW, WS_FORCED, WS_LEVEL, WS_MOVES, WS_PROPS, WS_N = 8 };

struct WfNet {   // one call; every pointer is device memory
    int B, W, scope, dry_run, max_rounds;
    u64 min_gain;
    uint16_t *rows;           // [PW]
    const uint8_t *rack_of;   // [B]
    const u64 *weight;        // [P]
    const u64 *wlead;         // [B]
    const uint16_t *meta;     // [P] e(p) | eligible slots << 8
    uint8_t *cur;             // [P] chosen slot, e(p) at the start
    uint8_t *slot;            // [P] slot proposed in this round | kWfWon
    u64 *key;                 // [P] key of this round's proposal, kWfNoKey = none
    const int32_t *cnt, *offl, *start, *list;   // the scenarios' affected / offline counts, their buckets
    int32_t *tlist, *trank;   // [PW] scratch per bucket: the brokers of T and their ranks, at start[g] * W
    u64 *scen;                // [6G]
    u64 *ctl;                 // [WC_N]
};

__global__ void k_wfo_wlead(int P, int W, const uint16_t *__restrict__ rows, const u64 *__restrict__ weight, u64 *__restrict__ wlead) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const u64 w = weight[p];
    if (w) atomicAdd(&wlead[rows[(size_t)p * W]], w);
}

// PROPOSE for partition p against the loads `load`: false when p proposes nothing (the eligible slots come from meta[p];
// wl_propose of kao_wleaders.hip takes every replica but the leader, so the two loops stay apart)
__device__ __forceinline__ bool wf_propose(const WfNet &n, int p, const u64 *load, int &a, int &b, int &slot, u64 &key) {
    const u64 w = n.weight[p];
    if (w == 0) return false;
    const uint16_t *row = n.rows + (size_t)p * n.W;
    const int mask = n.meta[p] >> 8, c = n.cur[p];
    a = row[c];
    u64 best = 0;
    slot = -1;
    for (int j = 1; j < n.W; ++j) {
        if (j == c || !((mask >> j) & 1)) continue;
        const int x = row[j];
        const u64 lx = load[x];
        if (slot < 0 || lx < best) { slot = j; best = lx; b = x; }
    }
    if (slot < 0) return false;
    const u64 la = load[a];
    if (!descent_gains(la, best, w, n.min_gain)) return false;
    key = DESCENT_KEY(la, w, p);
    return true;
}

// the largest v of the workgroup's lanes into the LDS word dst (read it after a barrier)
__device__ __forceinline__ void wf_max_to(u64 v, u64 *dst) {
    if (v > 0) atomicMax(dst, v);
}

__global__ __launch_bounds__(kFoSoloLarge) void k_wfo_solve(WfNet n) {
    extern __shared__ __attribute__((aligned(16))) u64 wf_lds[];
    __shared__ u64 s_part[kFoSoloLarge];
    __shared__ u64 sh[WS_N];
    __shared__ int32_t sh_nt, sh_cnt;
    const int g = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, B = n.B, W = n.W, na = n.cnt[g];
    const int32_t *list = n.list + n.start[g];
    u64 *load = wf_lds, *mk = wf_lds + B;
    if (tid < WS_N) sh[tid] = 0;
    if (tid == 0) { sh_nt = 0; sh_cnt = 0; }
    __syncthreads();
    {
        u64 mx = 0;
        for (int b = tid; b < B; b += NT)
            if (!fo_dead(b, g, n.scope, n.rack_of)) mx = max(mx, n.wlead[b]);
        wf_max_to(mx, &sh[WS_MAXLEAD]);
    }
    __syncthreads();
    if (na == 0) {   // nothing to choose: the peak is the survivors' largest preferred load, and so is the bound
        if (tid == 0) {
            u64 *o = n.scen + 6 * (size_t)g;
            const u64 m = sh[WS_MAXLEAD];
            o[0] = 0; o[1] = (u64)n.offl[g]; o[2] = m; o[3] = m; o[4] = m; o[5] = 0;
            atomicAdd(&n.ctl[WC_PROVEN], 1ull);
        }
        return;
    }
    // the start state j = e and peak_before
    for (int b = tid; b < B; b += NT) { load[b] = n.wlead[b]; mk[b] = kWfNoKey; }
    __syncthreads();
    for (int q = tid; q < na; q += NT) {
        const int p = list[q];
        const u64 w = n.weight[p];
        if (w) atomicAdd(&load[n.rows[(size_t)p * W + (n.meta[p] & 0xFF)]], w);
    }
    __syncthreads();
    {
        u64 mx = 0;
        for (int b = tid; b < B; b += NT)
            if (!fo_dead(b, g, n.scope, n.rack_of)) mx = max(mx, load[b]);
        wf_max_to(mx, &sh[WS_PEAK0]);
    }
    // ---- the rounds ----
    u64 props = 0, moves = 0;
    int rounds = 0, more = 0;
    for (;;) {
        int mine = 0;
        for (int q = tid; q < na; q += NT) {
            const int p = list[q];
            int a = 0, b = 0, slot = 0;
            u64 key = kWfNoKey;
            const bool prop = wf_propose(n, p, load, a, b, slot, key);
            n.key[p] = key;   // key[p], slot[p] and cur[p] are read back by this lane alone
            if (prop) {
                n.slot[p] = (uint8_t)slot;
                descent_bid<__HIP_MEMORY_SCOPE_WORKGROUP>(&mk[a], key);
                descent_bid<__HIP_MEMORY_SCOPE_WORKGROUP>(&mk[b], key);
                ++mine;
            }
        }
        if (!__syncthreads_or(mine)) break;
        if ((n.max_rounds > 0 && rounds >= n.max_rounds) || rounds >= kWfHardRounds) { more = 1; break; }
        ++rounds;
        props += (u64)mine;
        for (int q = tid; q < na; q += NT) {
            const int p = list[q];
            const u64 key = n.key[p];
            if (key == kWfNoKey) continue;
            const uint16_t *row = n.rows + (size_t)p * W;
            const int slot = n.slot[p];
            if (mk[row[n.cur[p]]] == key && mk[row[slot]] == key) n.slot[p] = (uint8_t)(slot | kWfWon);
        }
        __syncthreads();
        for (int q = tid; q < na; q += NT) {
            const int p = list[q];
            if (n.key[p] == kWfNoKey) continue;
            const uint16_t *row = n.rows + (size_t)p * W;
            const int s = n.slot[p], slot = s & (kWfWon - 1), a = row[n.cur[p]], b = row[slot];
            if (s & kWfWon) {   // no other winner touches a or b
                const u64 w = n.weight[p];
                load[a] -= w;
                load[b] += w;
                n.cur[p] = (uint8_t)slot;
                ++moves;
            }
            mk[a] = kWfNoKey;
            mk[b] = kWfNoKey;
        }
        __syncthreads();
    }
    __syncthreads();
    // (the certificate ranks a compacted set inside the workgroup; kao_wleaders.hip runs rank, histogram and scan as launches: not shared)
    // ---- peak_after; T = the brokers some affected partition is eligible for, compacted; their ranks ----
    {
        u64 mx = 0;
        for (int b = tid; b < B; b += NT)
            if (!fo_dead(b, g, n.scope, n.rack_of)) mx = max(mx, load[b]);
        wf_max_to(mx, &sh[WS_PEAK1]);
    }
    for (int q = tid; q < na; q += NT) {
        const int p = list[q], mask = n.meta[p] >> 8;
        for (int j = 1; j < W; ++j)
            if ((mask >> j) & 1) mk[n.rows[(size_t)p * W + j]] = 0;
    }
    __syncthreads();
    int32_t *tl = n.tlist + (size_t)n.start[g] * W, *tr = n.trank + (size_t)n.start[g] * W;
    for (int q = tid; q < na; q += NT) {
        const int p = list[q], mask = n.meta[p] >> 8;
        for (int j = 1; j < W; ++j) {
            if (!((mask >> j) & 1)) continue;
            const int b = n.rows[(size_t)p * W + j];
            if (atomicExch(&mk[b], 1ull) == 0ull) tl[atomicAdd(&sh_nt, 1)] = b;   // at most one slot of the bucket's na * W per broker
        }
    }
    __syncthreads();
    const int nt = sh_nt;
    for (int i = tid; i < nt; i += NT) {
        const int bi = tl[i];
        const u64 li = load[bi];
        int r = 0;
        for (int j = 0; j < nt; ++j) {
            const int bj = tl[j];
            const u64 lj = load[bj];
            r += (lj > li || (lj == li && bj < bi)) ? 1 : 0;
        }
        tr[i] = r;
    }
    __syncthreads();
    // the loads are done with: mk[b] = rank of b, hist[] (the load area) = Wlead by rank + the weight of the partitions by m_p
    u64 *hist = load;
    for (int i = tid; i < nt; i += NT) {
        const int b = tl[i], r = tr[i];
        mk[b] = (u64)r;
        hist[r] = n.wlead[b];
    }
    __syncthreads();
    {
        u64 t2 = 0;
        for (int q = tid; q < na; q += NT) {
            const int p = list[q], mask = n.meta[p] >> 8;
            const u64 w = n.weight[p];
            u64 m = 0, minw = kWfNoKey;
            for (int j = 1; j < W; ++j) {
                if (!((mask >> j) & 1)) continue;
                const int b = n.rows[(size_t)p * W + j];
                m = max(m, mk[b]);
                minw = min(minw, n.wlead[b]);
            }
            if (w) atomicAdd(&hist[m], w);
            t2 = max(t2, w + minw);
        }
        wf_max_to(t2, &sh[WS_MINW]);
    }
    __syncthreads();
    {   // A_k = hist[0] + .. + hist[k - 1]; max_k ceil(A_k / k)
        const int chunk = (nt + NT - 1) / NT, lo = min(nt, tid * chunk), hi = min(nt, lo + chunk);
        u64 sum = 0;
        for (int i = lo; i < hi; ++i) sum += hist[i];
        s_part[tid] = sum;
        __syncthreads();
        if (tid == 0) {   // exclusive prefix over the chunks
            u64 run = 0;
            for (int i = 0; i < NT; ++i) { const u64 x = s_part[i]; s_part[i] = run; run += x; }
        }
        __syncthreads();
        u64 run = s_part[tid], best = 0;
        for (int i = lo; i < hi; ++i) {
            run += hist[i];
            const u64 k = (u64)i + 1;
            best = max(best, run / k + (run % k != 0));
        }
        wf_max_to(best, &sh[WS_LEVEL]);
    }
    __syncthreads();
    // the forced loads: Wlead(b) + the weight of the partitions whose only eligible broker is b, by rank in the same area
    for (int i = tid; i < nt; i += NT) hist[tr[i]] = n.wlead[tl[i]];
    __syncthreads();
    for (int q = tid; q < na; q += NT) {
        const int p = list[q], mask = n.meta[p] >> 8;
        const u64 w = n.weight[p];
        if (w && (mask & (mask - 1)) == 0) atomicAdd(&hist[mk[n.rows[(size_t)p * W + (n.meta[p] & 0xFF)]]], w);
    }
    __syncthreads();
    {
        u64 mx = 0;
        for (int i = tid; i < nt; i += NT) mx = max(mx, hist[i]);
        wf_max_to(mx, &sh[WS_FORCED]);
    }
    // ---- the swaps ----
    {
        int moved = 0;
        for (int q = tid; q < na; q += NT) {
            const int p = list[q], e = n.meta[p] & 0xFF, c = n.cur[p];
            if (c == e) continue;
            ++moved;
            if (!n.dry_run) {
                uint16_t *row = n.rows + (size_t)p * W;
                const uint16_t x = row[e], y = row[c];
                row[e] = y;
                row[c] = x;
            }
        }
        if (moved) atomicAdd(&sh_cnt, moved);
        if (moves) atomicAdd(&sh[WS_MOVES], moves);
        if (props) atomicAdd(&sh[WS_PROPS], props);
    }
    __syncthreads();
    if (tid == 0) {
        const u64 lb = max(max(sh[WS_MAXLEAD], sh[WS_MINW]), max(sh[WS_FORCED], sh[WS_LEVEL]));
        u64 *o = n.scen + 6 * (size_t)g;
        o[0] = (u64)na; o[1] = (u64)n.offl[g]; o[2] = sh[WS_PEAK0]; o[3] = sh[WS_PEAK1]; o[4] = lb; o[5] = (u64)sh_cnt;
        atomicAdd(&n.ctl[WC_SCEN], 1ull);
        atomicAdd(&n.ctl[WC_ROUNDS], (u64)rounds);
        atomicAdd(&n.ctl[WC_MOVES], sh[WS_MOVES]);
        atomicAdd(&n.ctl[WC_PROPS], sh[WS_PROPS]);
        atomicAdd(&n.ctl[WC_MORE], (u64)more);
        if (sh[WS_PEAK1] == lb) atomicAdd(&n.ctl[WC_PROVEN], 1ull);
        atomicMax(&n.ctl[WC_MAXROUNDS], (u64)rounds);
        atomicAdd(&n.ctl[WC_REORDERED], (u64)sh_cnt);
        if (rounds >= kWfHardRounds) atomicAdd(&n.ctl[WC_ERR], 1ull);
    }
}

}  // namespace

extern "C" int kao_failover_order_weighted(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                                           uint16_t *rows, const uint64_t *weight, int32_t scope, uint64_t min_gain, int32_t max_rounds,
                                           int32_t dry_run, uint64_t *scen, int32_t *n_reordered, int32_t *status, int64_t stats[8]) {
    const std::string fn = "kao_failover_order_weighted: ";
    if (!weight || !status) return fail(KAO_ERR_INVALID, fn + "null pointer");
    int rc = validate_failover(fn, n_brokers, n_racks, rack_of, n_partitions, width, rows, scope, scen, n_reordered);
    if (rc) return rc;
    if ((rc = check_weight_sum(fn, n_partitions, weight))) return rc;
    if ((rc = require_init())) return rc;
    const int B = n_brokers, P = n_partitions, W = width, G = scope == 0 ? n_brokers : n_racks;
    const size_t PW = (size_t)P * W;

    // one arena: ctl32 i32[FS_N] | ctl u64[WC_N] | lead i32[B] | wlead u64[B] | cnt, off i32[G] (zeroed up to here) | start, fill i32[G] |
    //            scen u64[6G] | scen_of, list, claim i32[P] | tlist, trank i32[PW] | key, weight u64[P] | rows u16[PW] | meta u16[P] |
    //            cur, slot u8[P] | rack_of u8[B]
    Carve cv;
    const size_t o_ctl32 = cv.take<int32_t>(FS_N), o_ctl = cv.take<u64>(WC_N), o_lead = cv.take<int32_t>(B), o_wlead = cv.take<u64>(B),
                 o_cnt = cv.take<int32_t>(G), o_off = cv.take<int32_t>(G), zeroed = cv.end(), o_start = cv.take<int32_t>(G),
                 o_fill = cv.take<int32_t>(G), o_scen = cv.take<u64>(6 * (size_t)G), o_sof = cv.take<int32_t>(P), o_list = cv.take<int32_t>(P),
                 o_claim = cv.take<int32_t>(P), o_tlist = cv.take<int32_t>(PW), o_trank = cv.take<int32_t>(PW), o_key = cv.take<u64>(P),
                 o_w = cv.take<u64>(P), o_rows = cv.take<uint16_t>(PW), o_meta = cv.take<uint16_t>(P), o_cur = cv.take<uint8_t>(P),
                 o_slot = cv.take<uint8_t>(P), o_rack = cv.take<uint8_t>(B);
    CallBufs m;
    if ((rc = m.open(cv.end()))) return rc;
    hipStream_t st = m.stream;
    const FoScen d{m.at<int32_t>(o_lead), m.at<int32_t>(o_sof), m.at<int32_t>(o_cnt), m.at<int32_t>(o_off), m.at<int32_t>(o_start), m.at<int32_t>(o_fill),
                   m.at<int32_t>(o_list), m.at<int32_t>(o_claim), m.at<int32_t>(o_ctl32), m.at<uint16_t>(o_meta), m.at<uint8_t>(o_cur)};
    uint16_t *d_rows = m.at<uint16_t>(o_rows);
    uint8_t *d_rack = m.at<uint8_t>(o_rack);
    u64 *d_wlead = m.at<u64>(o_wlead), *d_w = m.at<u64>(o_w);

    HIP_TRY(hipMemsetAsync(m.arena, 0, zeroed, st));
    HIP_TRY(hipMemcpyAsync(d_rack, rack_of, (size_t)B, hipMemcpyHostToDevice, st));
    if (P) {
        HIP_TRY(hipMemcpyAsync(d_rows, rows, PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_w, weight, (size_t)P * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    int launches = 0, max_n = 0, threads = 0;
    if (P) {
        k_wfo_wlead<<<grid_for(P, kFoThreads), kFoThreads, 0, st>>>(P, W, d_rows, d_w, d_wlead);
        ++launches;
    }
    const size_t lds = 2 * (size_t)B * sizeof(u64);
    if ((rc = fo_prelude(st, P, W, G, scope, d_rows, d_rack, d, reinterpret_cast<const void *>(k_wfo_solve), lds, 32 * 1024, &launches, &max_n, &threads)))
        return rc;
    WfNet n;
    n.B = B; n.W = W; n.scope = scope; n.dry_run = dry_run; n.max_rounds = max_rounds; n.min_gain = min_gain;
    n.rows = d_rows; n.rack_of = d_rack; n.weight = d_w; n.wlead = d_wlead; n.meta = d.meta; n.cur = d.cur; n.slot = m.at<uint8_t>(o_slot);
    n.key = m.at<u64>(o_key); n.cnt = d.cnt; n.offl = d.off; n.start = d.start; n.list = d.list; n.tlist = m.at<int32_t>(o_tlist);
    n.trank = m.at<int32_t>(o_trank); n.scen = m.at<u64>(o_scen); n.ctl = m.at<u64>(o_ctl);
    k_wfo_solve<<<(unsigned)G, threads, lds, st>>>(n);
    HIP_TRY(hipGetLastError());
    ++launches;
    u64 ctl[WC_N];
    HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(scen, n.scen, (size_t)G * 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctl[WC_ERR]) return fail(KAO_ERR_HIP, fn + "the rounds did not finish");
    if (!dry_run && P && ctl[WC_REORDERED]) {
        HIP_TRY(hipMemcpyAsync(rows, d_rows, PW * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_reordered = (int32_t)ctl[WC_REORDERED];
    *status = ctl[WC_PROVEN] == (u64)G ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
    if (stats) {
        stats[0] = (int64_t)ctl[WC_SCEN]; stats[1] = (int64_t)ctl[WC_ROUNDS]; stats[2] = (int64_t)ctl[WC_MOVES]; stats[3] = (int64_t)ctl[WC_PROPS];
        stats[4] = launches; stats[5] = (int64_t)ctl[WC_MORE]; stats[6] = (int64_t)ctl[WC_PROVEN]; stats[7] = (int64_t)ctl[WC_MAXROUNDS];
    }
    return KAO_OK;
}
