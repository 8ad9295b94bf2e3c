// kao_wleaders.hip -- kao_balance_leaders_weighted: the preferred leaders of all topics chosen so that the traffic a broker leads,
// W(b) = sum of weight[p] over the partitions b leads, has a low peak; replica sets kept.  Kernels and the C
// entry point.
//
// Minimising the peak is restricted-assignment makespan (NP-hard), so this is a deterministic parallel DESCENT with a CERTIFICATE.
// State: a leader slot j(p) per partition (0 at the start) and the loads W.  A ROUND uses the loads as they stand at its start:
//   1. every partition with weight > 0 and two replicas or more takes b* = its other replica with the lowest load (ties: the lowest
//      slot index) and, with a = its leader, PROPOSES a -> b* iff W(b*) + weight + min_gain < W(a);
//   2. key(p) = (0xFFFF - code(W(a))) << 48 | (0xFFFF - code(weight[p])) << 32 | p, code = wave_bytes_code: heaviest source first,
//      then the heaviest partition, then the lowest index;
//   3. a proposal WINS iff its key is the lowest of all proposals that touch a (as source or destination) and likewise at b*: one
//      64-bit atomicMin per participant into minkey[b].  Winners share no broker, so W(a) -= w, W(b*) += w, j(p) = that slot are
//      plain stores;
//   4. until a round has no proposal (or max_rounds rounds have run).
// The globally lowest key always wins, every move lowers sum W^2 strictly and leaves both loads below the old W(a): the rounds end
// and the peak never rises.
// The snapshot "loads as of the round's start" is kept by splitting a round in two: PROPOSE reads the loads and writes only key[p],
// slot[p] and the minkey row; APPLY reads key[p], slot[p] and the minkey row and writes the loads.  On the multi-launch path the two
// are two kernels (the kernel boundary is the barrier), two minkey rows rotate (apply of round r clears the row of round r + 1), and
// the host reads the rounds' proposal counts every kWlBatch rounds; rounds after the first empty one change nothing.  On the
// single-workgroup path (loads and both minkey rows in LDS, 24 bytes per broker) one launch runs every round with two barriers per
// round.  Both paths follow the one definition and give identical bytes.
// The certificate: brokers ranked by final load descending (ties: index ascending), m_p = the largest rank in row p, A_k = sum of
// weight[p] over m_p < k, forced(b) = the weight of the rows with one replica at b; lower bound = max(max weight, max forced,
// max_k ceil(A_k / k)), valid for ANY leader choice: a partition with every replica among the k highest-ranked brokers is led by
// one of them, so one of them carries at least their average.  Rank (all pairs, tiled through LDS), one pass over the rows into a
// u64 histogram over m_p, one scan.  Integers only.
// kao_balance_leaders_weighted_exchange is the same call with a second kind of round, run when a round has
// no move proposal: two partitions on one broker pair swap their leaders (see EXCHANGE rounds below).  Its state is WlxNet, the plain
// call's WlNet and the pair index.  The two calls share every text: a round's apply kernel and the single-workgroup kernel are
// templates on X, the exchange call, and take WlxNet or WlNet; the instantiations without X hold nothing of the exchange.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "kao_host.h"
#include "kao_plan_dev.h"   // DESCENT_KEY, descent_gains, descent_bid, lane_count_to, wave_max_to, rank_ahead, swap_leader

namespace {

constexpr int kWlThreads = 256;
constexpr int kWlBatch = 32;            // rounds enqueued between two reads of the proposal counts
constexpr int kWlOneThreads = 1024;     // the single workgroup
constexpr int kWlOneMaxB = 2048;        // ... holds loads + two minkey rows in LDS: 24 bytes per broker, 48 KiB
constexpr int kWlOneMaxP = 4096;        // ... and is chosen up to this many partitions (threshold)
constexpr int kWlHardRounds = 1 << 26;  // no descent gets here; a guard against an endless loop
constexpr u64 kWlNoKey = ~0ull;
enum { U_PEAK0 = 0, U_PEAK1, U_MOVES, U_PROPS, U_ROUNDS, U_MAXW, U_FORCED, U_LEVEL, U_LEVELK, U_CHANGED, U_LEADING, U_MORE, U_XROUNDS, U_XCH, U_XPROPS, U_N = 16 };

thread_local int t_wl_path = 0;   // kao_wleaders_test_path: 0 = by size, 1 = single workgroup, 2 = multi-launch

struct WlNet {   // one call; every pointer is device memory
    int P, W, B;
    u64 min_gain;
    const uint16_t *rows;   // [PW]
    const u64 *weight;      // [P]
    uint8_t *lead;          // [P] chosen slot
    uint8_t *slot;          // [P] slot proposed in this round
    u64 *key;               // [P] key of this round's proposal, kWlNoKey = none
    u64 *load;              // [B]
    u64 *mk;                // [2][B] minkey rows
    u64 *ctl;               // [U_N]
};

struct WlxNet {   // one call of kao_balance_leaders_weighted_exchange: the plain call's state and the pair index
    WlNet n;
    int NP;                   // slot pairs of a row: W (W - 1) / 2
    const uint32_t *ent;      // [entries] the partitions of the pair index: one segment per broker pair, each in the order PI
    const uint32_t *seg_lo;   // [segments + 1] where a segment starts
    const uint32_t *pseg;     // [P * NP] the segment of (partition, slot pair); unused where weight is 0
    uint32_t *partner;        // [P] the y of this round's exchange proposal
    uint16_t *pa, *pc;        // [P] its two brokers: apply never reads lead[]
};

// the plain call's state inside the argument of a kernel of either call
__device__ __forceinline__ const WlNet &wl_net(const WlNet &n) { return n; }
__device__ __forceinline__ const WlNet &wl_net(const WlxNet &x) { return x.n; }

// Step 1 and 2 for partition p against the loads `load`: false when p proposes nothing (every replica but the leader is eligible;
// wf_propose of kao_wfailover.hip reads its eligible slots from a mask, so the two loops stay apart)
__device__ inline bool wl_propose(const WlNet &n, int p, const u64 *load, int &a, int &b, int &slot, u64 &key) {
    const u64 w = n.weight[p];
    if (w == 0) return false;
    const uint16_t *row = n.rows + (size_t)p * n.W;
    const int l = n.lead[p];
    a = row[l];
    u64 best = 0;
    slot = -1;
    for (int j = 0; j < n.W; ++j) {
        const int x = row[j];
        if (x == KAO_NONE) break;
        if (j == l) continue;
        const u64 wx = load[x];
        if (slot < 0 || wx < best) { slot = j; best = wx; b = x; }
    }
    if (slot < 0) return false;
    const u64 wa = load[a];
    if (!descent_gains(wa, best, w, n.min_gain)) return false;
    key = DESCENT_KEY(wa, w, p);
    return true;
}

// ---- once per call ------------------------------------------------------------------------------------------------------------------
__global__ void k_wl_init(WlNet n, u64 *__restrict__ forced) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    u64 w = 0;
    if (p < n.P) {
        w = n.weight[p];
        n.lead[p] = 0;
        n.key[p] = kWlNoKey;
        const uint16_t *row = n.rows + (size_t)p * n.W;
        if (w) {
            atomicAdd(&n.load[row[0]], w);
            if (n.W == 1 || row[1] == KAO_NONE) atomicAdd(&forced[row[0]], w);
        }
    }
    wave_max_to(w, &n.ctl[U_MAXW]);
}

__global__ void k_wl_max(int B, const u64 *__restrict__ x, u64 *__restrict__ dst) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    wave_max_to(b < B ? x[b] : 0, dst);
}

// ---- a round ----------------------------------------------------------------------------------------------------------------------
// What a propose found for partition p is posted: key[p] (kWlNoKey when `prop` is false) and, for a proposal, slot[p], a bid at both of
// its brokers in the minkey row of round r (mk = both rows) and one more in `posted`.  Scope as descent_bid has it; rows in LDS
// (_WORKGROUP) take the plain atomicMin, without descent_bid's load.
// (`posted` is counted here, in the branch that bids, and the row is taken after the stores: counted by the caller from a returned
// flag, the loop of the single workgroup gains a second test of it and selects)
template <int Scope>
__device__ __forceinline__ void wl_post(const WlNet &n, int p, bool prop, u64 key, int slot, u64 *mk, int r, int a, int b, int &posted) {
    n.key[p] = key;
    if (!prop) return;
    n.slot[p] = (uint8_t)slot;
    u64 *row = mk + (size_t)(r & 1) * n.B;
    if constexpr (Scope == __HIP_MEMORY_SCOPE_WORKGROUP) {
        atomicMin(&row[a], key);
        atomicMin(&row[b], key);
    } else {
        descent_bid<Scope>(&row[a], key);
        descent_bid<Scope>(&row[b], key);
    }
    ++posted;
}

// the PROPOSE of a round on the multi-launch path
__global__ void k_wl_propose(WlNet n, int r, uint32_t *__restrict__ count) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    int prop = 0;
    if (p < n.P) {
        int a = 0, b = 0, slot = 0;
        u64 key = kWlNoKey;
        const bool found = wl_propose(n, p, n.load, a, b, slot, key);
        wl_post<__HIP_MEMORY_SCOPE_AGENT>(n, p, found, key, slot, n.mk, r, a, b, prop);
    }
    lane_count_to(prop != 0, count);
}

// ---- EXCHANGE rounds -----------------------------------------------------------------------------------------
// A round without a move proposal is an EXCHANGE round: x (led by a) and y (led by c, lighter than x), both rows holding both
// brokers, swap leaders: W(a) -= delta, W(c) += delta, delta = weight[x] - weight[y].  The rows of a broker pair are one segment of
// the pair index, heaviest first, so x finds its partner by a binary search and a short scan, never by comparing pairs.
constexpr uint32_t kWlxNoY = 0xFFFFFFFFu;

// first e in [lo, hi) whose weight fails `pred` (pred holds on a prefix: the segment is in weight order, heaviest first)
template <class Pred>
__device__ __forceinline__ uint32_t wlx_first_not(const WlxNet &x, uint32_t lo, uint32_t hi, Pred pred) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pred(x.n.weight[x.ent[mid]])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The exchange proposal of partition p against the loads `load`: false when it has none.  Reads loads and lead[], writes nothing.
__device__ inline bool wlx_propose(const WlxNet &x, int p, const u64 *load, int &a, int &c, int &slot, uint32_t &y, u64 &key) {
    const WlNet &n = x.n;
    const u64 w = n.weight[p], mg = n.min_gain;
    if (w == 0) return false;
    const uint16_t *row = n.rows + (size_t)p * n.W;
    const int l = n.lead[p];
    a = row[l];
    const u64 wa = load[a];
    for (uint32_t done = 1u << l;;) {   // the other replicas by load ascending, ties to the lowest slot
        int j = -1;
        u64 wc = 0;
        for (int s = 0; s < n.W; ++s) {
            const int b = row[s];
            if (b == KAO_NONE) break;
            if (done >> s & 1u) continue;
            const u64 v = load[b];
            if (j < 0 || v < wc) { j = s; wc = v; }
        }
        if (j < 0 || wc >= wa) return false;   // D <= 0, and no later candidate has a larger D
        done |= 1u << j;
        const u64 D = wa - wc;
        if (D <= mg) return false;             // delta + min_gain < D has no delta >= 1
        c = row[j];
        const int i0 = min(l, j), i1 = max(l, j);
        const uint32_t seg = x.pseg[(size_t)p * x.NP + i0 * (2 * n.W - i0 - 1) / 2 + (i1 - i0 - 1)];
        const uint32_t lo = x.seg_lo[seg], hi = x.seg_lo[seg + 1];
        // the split: members before s have 2 weight > 2 w - D (delta below D / 2); every sum stays below 2^64
        const uint32_t s = wlx_first_not(x, lo, hi, [&](u64 wq) { return 2 * wq + D > 2 * w; });
        // ... clamped into the passing run: for 2 min_gain >= D the members next to the split fail delta + min_gain < D
        const uint32_t h = mg < D - mg ? s : wlx_first_not(x, lo, s, [&](u64 wq) { return wq >= w || D - (w - wq) > mg; });
        uint32_t y_hi = kWlxNoY, y_lo = kWlxNoY;
        u64 d_hi = 0, d_lo = 0;
        for (uint32_t e = h; e-- > lo;) {      // heavier and heavier: until delta <= 0
            const uint32_t q = x.ent[e];
            const u64 wq = n.weight[q];
            if (wq >= w) break;
            if (n.rows[(size_t)q * n.W + n.lead[q]] == c) { y_hi = q; d_hi = w - wq; break; }
        }
        for (uint32_t e = s; e < hi; ++e) {    // lighter and lighter: until delta + min_gain >= D (weight < w from s on)
            const uint32_t q = x.ent[e];
            const u64 d = w - n.weight[q];
            if (d >= D || D - d <= mg) break;
            if (n.rows[(size_t)q * n.W + n.lead[q]] == c) { y_lo = q; d_lo = d; break; }
        }
        if (y_hi == kWlxNoY && y_lo == kWlxNoY) continue;
        const bool take_hi = y_hi != kWlxNoY && (y_lo == kWlxNoY || D - 2 * d_hi < 2 * d_lo - D);   // a tie goes to y_lo
        y = take_hi ? y_hi : y_lo;
        slot = j;
        key = DESCENT_KEY(wa, take_hi ? d_hi : d_lo, p);
        return true;
    }
}

// apply of a MOVE proposal against the round's minkey row `mine`: a winner (no other winner touches a or b) moves its leader and adds 1
// to `won`, inside the branch that moves (see wl_post)
__device__ __forceinline__ void wl_apply_move(const WlNet &n, int p, u64 key, const u64 *mine, u64 *load, u64 &won) {
    const uint16_t *row = n.rows + (size_t)p * n.W;
    const int slot = n.slot[p], a = row[n.lead[p]], b = row[slot];
    if (mine[a] != key || mine[b] != key) return;
    const u64 w = n.weight[p];
    load[a] -= w;
    load[b] += w;
    n.lead[p] = (uint8_t)slot;
    ++won;
}

// apply of an EXCHANGE proposal, counted likewise: its brokers come from what propose stored, because a winner writes lead[y] of another
// partition
__device__ __forceinline__ void wlx_apply_swap(const WlxNet &x, int p, u64 key, const u64 *mine, u64 *load, u64 &won) {
    const WlNet &n = x.n;
    const int a = x.pa[p], c = x.pc[p];
    if (mine[a] != key || mine[c] != key) return;   // no other winner touches a or c, x or y
    const uint32_t y = x.partner[p];
    const u64 d = n.weight[p] - n.weight[y];
    load[a] -= d;
    load[c] += d;
    n.lead[p] = n.slot[p];
    const uint16_t *ry = n.rows + (size_t)y * n.W;
    int ja = 0;
    while (ja < n.W - 1 && ry[ja] != a) ++ja;
    n.lead[y] = (uint8_t)ja;
    ++won;
}

// what an exchange proposal stores beside wl_post
__device__ __forceinline__ void wlx_post_pair(const WlxNet &x, int p, uint32_t y, int a, int c) {
    x.partner[p] = y;
    x.pa[p] = (uint16_t)a;
    x.pc[p] = (uint16_t)c;
}

// enqueued behind every k_wl_propose: returns at once when that round has a move proposal
__global__ void k_wlx_propose(WlxNet x, int r, const uint32_t *__restrict__ moves, uint32_t *__restrict__ count) {
    if (*moves) return;
    const WlNet &n = x.n;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    int prop = 0;
    if (p < n.P) {   // key[p] is kWlNoKey: k_wl_propose found nothing
        int a = 0, c = 0, slot = 0;
        uint32_t y = 0;
        u64 key = kWlNoKey;
        if (wlx_propose(x, p, n.load, a, c, slot, y, key)) {
            wlx_post_pair(x, p, y, a, c);
            wl_post<__HIP_MEMORY_SCOPE_AGENT>(n, p, true, key, slot, n.mk, r, a, c, prop);
        }
    }
    lane_count_to(prop != 0, count);
}

// ---- the apply of a round, and every round in one launch: both calls, X = the exchange call -------------------------------------------
// `moves` (X only) = the round's move proposals: 0 in an exchange round
template <bool X>
__global__ void k_wl_apply(std::conditional_t<X, WlxNet, WlNet> net, int r, const uint32_t *__restrict__ moves) {
    const WlNet &n = wl_net(net);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    {   // the row of round r + 1 was last read by the apply of round r - 1
        u64 *clr = n.mk + (size_t)((r + 1) & 1) * n.B;
        for (int e = p; e < n.B; e += gridDim.x * blockDim.x) clr[e] = kWlNoKey;
    }
    bool move = true;
    if constexpr (X) move = *moves != 0;
    u64 won = 0;   // 1: the proposal of this lane won
    if (p < n.P) {
        const u64 key = n.key[p];
        if (key != kWlNoKey) {
            const u64 *mine = n.mk + (size_t)(r & 1) * n.B;
            if (move) wl_apply_move(n, p, key, mine, n.load, won);
            else if constexpr (X) wlx_apply_swap(net, p, key, mine, n.load, won);
        }
    }
    lane_count_to(won != 0, &n.ctl[move ? U_MOVES : U_XCH]);
}

// one workgroup, loads and minkey rows in LDS (X: the pair index in global memory)
template <bool X>
__global__ __launch_bounds__(kWlOneThreads) void k_wl_one(std::conditional_t<X, WlxNet, WlNet> net, int max_rounds) {
    extern __shared__ u64 wl_lds[];
    const WlNet &n = wl_net(net);
    u64 *load = wl_lds, *mk = wl_lds + n.B;
    const int tid = threadIdx.x;
    for (int b = tid; b < n.B; b += kWlOneThreads) {
        load[b] = n.load[b];
        mk[b] = kWlNoKey;
        mk[n.B + b] = kWlNoKey;
    }
    __syncthreads();
    u64 props = 0, moves = 0;
    int rounds = 0, more = 0;
    [[maybe_unused]] u64 xprops = 0, swaps = 0;   // X
    [[maybe_unused]] int xrounds = 0;
    for (int r = 0; r < kWlHardRounds; ++r) {
        u64 *row = mk + (size_t)(r & 1) * n.B, *other = mk + (size_t)((r + 1) & 1) * n.B;
        int mine = 0;
        for (int p = tid; p < n.P; p += kWlOneThreads) {
            int a = 0, b = 0, slot = 0;
            u64 key = kWlNoKey;
            const bool prop = wl_propose(n, p, load, a, b, slot, key);
            wl_post<__HIP_MEMORY_SCOPE_WORKGROUP>(n, p, prop, key, slot, mk, r, a, b, mine);
        }
        const bool move = __syncthreads_or(mine) != 0;
        if constexpr (X) {
            if (!move) {   // an EXCHANGE round: the lead[] of other partitions was written before the barrier that ended the last round
                for (int p = tid; p < n.P; p += kWlOneThreads) {
                    int a = 0, c = 0, slot = 0;
                    uint32_t y = 0;
                    u64 key = kWlNoKey;
                    if (!wlx_propose(net, p, load, a, c, slot, y, key)) continue;
                    wlx_post_pair(net, p, y, a, c);
                    wl_post<__HIP_MEMORY_SCOPE_WORKGROUP>(n, p, true, key, slot, mk, r, a, c, mine);
                }
                if (!__syncthreads_or(mine)) break;
            }
        } else if (!move) {
            break;
        }
        if (max_rounds > 0 && r >= max_rounds) { more = 1; break; }
        ++rounds;
        props += (u64)mine;
        if (X && !move) { ++xrounds; xprops += (u64)mine; }
        for (int p = tid; p < n.P; p += kWlOneThreads) {
            const u64 key = n.key[p];
            if (key == kWlNoKey) continue;
            if constexpr (X) {
                if (!move) {
                    wlx_apply_swap(net, p, key, row, load, swaps);
                    continue;
                }
            }
            wl_apply_move(n, p, key, row, load, moves);
        }
        for (int b = tid; b < n.B; b += kWlOneThreads) other[b] = kWlNoKey;
        __syncthreads();
    }
    __syncthreads();
    for (int b = tid; b < n.B; b += kWlOneThreads) n.load[b] = load[b];
    if (props) atomicAdd(&n.ctl[U_PROPS], props);
    if (moves) atomicAdd(&n.ctl[U_MOVES], moves);
    if constexpr (X) {
        if (xprops) atomicAdd(&n.ctl[U_XPROPS], xprops);
        if (swaps) atomicAdd(&n.ctl[U_XCH], swaps);
    }
    if (tid == 0) {
        n.ctl[U_ROUNDS] = (u64)rounds;
        if constexpr (X) n.ctl[U_XROUNDS] = (u64)xrounds;
        n.ctl[U_MORE] = (u64)more;
    }
}

// ---- the certificate and the result -------------------------------------------------------------------------------------------------
// (rank, histogram and scan in three launches over all brokers; k_wfo_solve of kao_wfailover.hip ranks a compacted set inside its
// workgroup and reuses its LDS for the histogram: not shared)
// rank[b] = brokers ahead of b by (load descending, index ascending); the peak on the way
__global__ __launch_bounds__(kWlThreads) void k_wl_rank(int B, const u64 *__restrict__ load, int32_t *__restrict__ rank, u64 *__restrict__ peak) {
    const int b = blockIdx.x * kWlThreads + threadIdx.x;
    const u64 mine = b < B ? load[b] : 0;
    const int r = rank_ahead<kWlThreads, false>(B, b, mine, 1, load, nullptr);
    if (b < B) rank[b] = r;
    wave_max_to(mine, peak);
}

// one lane per partition: the row's largest rank into the histogram, the leader's count, the swap
__global__ void k_wl_finish(WlNet n, const int32_t *__restrict__ rank, u64 *__restrict__ hist, int32_t *__restrict__ led,
                            uint16_t *__restrict__ rows, int dry_run) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool ch = false;
    if (p < n.P) {
        uint16_t *row = rows + (size_t)p * n.W;
        const int l = n.lead[p];
        int m = 0;
        for (int j = 0; j < n.W && row[j] != KAO_NONE; ++j) m = max(m, rank[row[j]]);
        const u64 w = n.weight[p];
        if (w) atomicAdd(&hist[m], w);
        atomicAdd(&led[row[l]], 1);
        ch = l != 0;
        if (ch && !dry_run) swap_leader(row, l);
    }
    lane_count_to(ch, &n.ctl[U_CHANGED]);
}

// one workgroup: A_k = hist[0] + .. + hist[k - 1], the level-set term max_k ceil(A_k / k) with the lowest k that attains it, the
// largest forced load, the brokers that lead something
__global__ __launch_bounds__(kWlThreads) void k_wl_scan(int B, const u64 *__restrict__ hist, const u64 *__restrict__ forced,
                                                         const int32_t *__restrict__ led, u64 *__restrict__ ctl) {
    __shared__ u64 s_sum[kWlThreads], s_best[kWlThreads], s_forced[kWlThreads];
    __shared__ int s_k[kWlThreads], s_lead[kWlThreads];
    const int t = threadIdx.x, chunk = (B + kWlThreads - 1) / kWlThreads, lo = min(B, t * chunk), hi = min(B, lo + chunk);
    u64 sum = 0;
    for (int i = lo; i < hi; ++i) sum += hist[i];
    s_sum[t] = sum;
    __syncthreads();
    if (t == 0) {   // exclusive prefix over the chunks
        u64 run = 0;
        for (int i = 0; i < kWlThreads; ++i) { const u64 x = s_sum[i]; s_sum[i] = run; run += x; }
    }
    __syncthreads();
    u64 run = s_sum[t], best = 0, fmax = 0;
    int bestk = 0, nlead = 0;
    for (int i = lo; i < hi; ++i) {
        run += hist[i];
        const u64 k = (u64)i + 1, v = run / k + (run % k != 0);
        if (v > best) { best = v; bestk = i + 1; }
        fmax = max(fmax, forced[i]);
        nlead += led[i] > 0;
    }
    s_best[t] = best; s_k[t] = bestk; s_forced[t] = fmax; s_lead[t] = nlead;
    __syncthreads();
    if (t == 0) {
        best = 0; bestk = 0; fmax = 0; nlead = 0;
        for (int i = 0; i < kWlThreads; ++i) {   // chunks ascend in k: a strict comparison keeps the lowest k
            if (s_best[i] > best) { best = s_best[i]; bestk = s_k[i]; }
            fmax = max(fmax, s_forced[i]);
            nlead += s_lead[i];
        }
        ctl[U_LEVEL] = best; ctl[U_LEVELK] = (u64)bestk; ctl[U_FORCED] = fmax; ctl[U_LEADING] = (u64)nlead;
    }
}

int validate_weighted(const std::string &fn, int32_t B, int32_t P, int32_t W, const uint16_t *rows, const uint64_t *weight, const int32_t *n_changed,
                      const uint64_t *peak_before, const uint64_t *peak_after, const uint64_t *lower_bound, const int32_t *status) {
    if (!rows || !weight || !n_changed || !peak_before || !peak_after || !lower_bound || !status) return fail(KAO_ERR_INVALID, fn + "null pointer");
    int rc = check_dims(fn, B, P, W);
    if (!rc) rc = check_slot_cap(fn, P, W);
    if (!rc) rc = check_rows(fn, B, P, W, rows);
    return rc ? rc : check_weight_sum(fn, P, weight);
}

// ---- the pair index of the exchange call, built on the host once per call -----------------------------------------------------------
// One entry per partition with weight > 0 and per unordered pair of its replicas, sorted by (lower broker, higher broker, position in
// PI): every broker pair is then one segment in weight order.  The entries are made in the order PI, so two stable counting passes
// over the broker indices (higher, then lower) sort them; pseg is the table from (partition, slot pair) to its segment.
struct WlxIndex {
    int NP = 0;
    std::vector<uint32_t> ent, seg_lo, pseg;
};

thread_local int64_t t_wlx_setup_us = 0;   // kao_wleaders_last_setup_us

void wlx_build_index(int B, int P, int W, const uint16_t *rows, const uint64_t *weight, WlxIndex &ix) {
    ix.NP = W * (W - 1) / 2;
    ix.pseg.assign((size_t)P * ix.NP, 0);
    std::vector<uint32_t> pi;
    for (int p = 0; p < P; ++p)
        if (weight[p] && W >= 2 && rows[(size_t)p * W + 1] != KAO_NONE) pi.push_back((uint32_t)p);
    std::sort(pi.begin(), pi.end(), [&](uint32_t x, uint32_t y) { return weight[x] != weight[y] ? weight[x] > weight[y] : x < y; });
    struct Ent { uint32_t pair, at; };   // lower broker << 16 | higher broker; partition << 5 | slot pair
    std::vector<Ent> e, t;
    for (uint32_t p : pi) {
        const uint16_t *row = rows + (size_t)p * W;
        for (int i = 0; i < W && row[i] != KAO_NONE; ++i)
            for (int j = i + 1; j < W && row[j] != KAO_NONE; ++j)
                e.push_back({(uint32_t)std::min(row[i], row[j]) << 16 | std::max(row[i], row[j]), p << 5 | (uint32_t)(i * (2 * W - i - 1) / 2 + (j - i - 1))});
    }
    t.resize(e.size());
    for (int shift = 0; shift <= 16; shift += 16) {
        std::vector<uint32_t> at((size_t)B + 1, 0);
        for (const Ent &v : e) ++at[(v.pair >> shift & 0xFFFFu) + 1];
        for (int b = 0; b < B; ++b) at[(size_t)b + 1] += at[b];
        for (const Ent &v : e) t[at[v.pair >> shift & 0xFFFFu]++] = v;
        e.swap(t);
    }
    ix.ent.resize(e.size());
    for (size_t i = 0; i < e.size(); ++i) {
        if (i == 0 || e[i].pair != e[i - 1].pair) ix.seg_lo.push_back((uint32_t)i);
        ix.ent[i] = e[i].at >> 5;
        ix.pseg[(size_t)(e[i].at >> 5) * ix.NP + (e[i].at & 31u)] = (uint32_t)ix.seg_lo.size() - 1;
    }
    ix.seg_lo.push_back((uint32_t)e.size());
}

// Both entry points: `exchange` adds the pair index, k_wlx_propose, the X instantiations of the two templates and stats[8..11].
int wl_call(bool exchange, const std::string &fn, int32_t n_brokers, int32_t n_partitions, int32_t width, uint16_t *rows, const uint64_t *weight,
            uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_changed, uint64_t *peak_before, uint64_t *peak_after,
            uint64_t *lower_bound, int32_t *status, int64_t *stats) {
    int rc = validate_weighted(fn, n_brokers, n_partitions, width, rows, weight, n_changed, peak_before, peak_after, lower_bound, status);
    if (rc) return rc;
    if ((rc = require_init())) return rc;
    const int B = n_brokers, P = n_partitions, W = width, PW = P * W;
    const bool one = t_wl_path == 1 || (t_wl_path == 0 && B <= kWlOneMaxB && P <= kWlOneMaxP);
    if (one && B > kWlOneMaxB) return fail(KAO_ERR_UNSUPPORTED, fn + "the single-workgroup path holds at most " + std::to_string(kWlOneMaxB) + " brokers");
    WlxIndex ix;
    if (exchange) {
        const double t0 = now_s();
        wlx_build_index(B, P, W, rows, weight, ix);
        t_wlx_setup_us = (int64_t)((now_s() - t0) * 1e6);
    }
    const int ncnt = exchange ? 2 * kWlBatch : kWlBatch;   // the rounds' move proposals, then their exchange proposals

    // one arena: ctl u64[U_N] | count u32[ncnt] | load, forced, hist u64[B] | led, rank i32[B] (zeroed up to here) | mk u64[2B]
    //            (all ones) | key, weight u64[P] | rows u16[PW] | lead, slot u8[P] | the exchange call's: ent, seg_lo, pseg, partner
    //            u32 | pa, pc u16[P]
    Carve cv;
    const size_t o_ctl = cv.take<u64>(U_N), o_cnt = cv.take<uint32_t>(ncnt), o_load = cv.take<u64>(B), o_forced = cv.take<u64>(B),
                 o_hist = cv.take<u64>(B), o_led = cv.take<int32_t>(B), o_rank = cv.take<int32_t>(B), zeroed = cv.end(),
                 o_mk = cv.take<u64>(2 * (size_t)B), o_key = cv.take<u64>(P), o_w = cv.take<u64>(P), o_rows = cv.take<uint16_t>(PW),
                 o_lead = cv.take<uint8_t>(P), o_slot = cv.take<uint8_t>(P);
    size_t o_ent = 0, o_seg = 0, o_pseg = 0, o_partner = 0, o_pa = 0, o_pc = 0;
    if (exchange) {
        o_ent = cv.take<uint32_t>(ix.ent.size()); o_seg = cv.take<uint32_t>(ix.seg_lo.size()); o_pseg = cv.take<uint32_t>(ix.pseg.size());
        o_partner = cv.take<uint32_t>(P); o_pa = cv.take<uint16_t>(P); o_pc = cv.take<uint16_t>(P);
    }
    CallBufs m;
    if ((rc = m.open(cv.end()))) return rc;
    hipStream_t st = m.stream;
    uint16_t *d_rows = m.at<uint16_t>(o_rows);
    uint32_t *d_cnt = m.at<uint32_t>(o_cnt);
    int32_t *d_led = m.at<int32_t>(o_led), *d_rank = m.at<int32_t>(o_rank);
    u64 *d_forced = m.at<u64>(o_forced), *d_hist = m.at<u64>(o_hist);
    WlxNet x;
    WlNet &n = x.n;
    n.P = P; n.W = W; n.B = B; n.min_gain = min_gain;
    n.rows = d_rows; n.weight = m.at<u64>(o_w); n.lead = m.at<uint8_t>(o_lead); n.slot = m.at<uint8_t>(o_slot); n.key = m.at<u64>(o_key);
    n.load = m.at<u64>(o_load); n.mk = m.at<u64>(o_mk); n.ctl = m.at<u64>(o_ctl);
    x.NP = ix.NP; x.ent = m.at<uint32_t>(o_ent); x.seg_lo = m.at<uint32_t>(o_seg); x.pseg = m.at<uint32_t>(o_pseg);
    x.partner = m.at<uint32_t>(o_partner); x.pa = m.at<uint16_t>(o_pa); x.pc = m.at<uint16_t>(o_pc);

    HIP_TRY(hipMemsetAsync(m.arena, 0, zeroed, st));
    HIP_TRY(hipMemsetAsync(n.mk, 0xFF, 2 * (size_t)B * sizeof(u64), st));
    if (P) {
        HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<u64>(o_w), weight, (size_t)P * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    if (exchange) {
        if (!ix.ent.empty()) HIP_TRY(hipMemcpyAsync(m.at<uint32_t>(o_ent), ix.ent.data(), ix.ent.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<uint32_t>(o_seg), ix.seg_lo.data(), ix.seg_lo.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (!ix.pseg.empty()) HIP_TRY(hipMemcpyAsync(m.at<uint32_t>(o_pseg), ix.pseg.data(), ix.pseg.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    const unsigned pblocks = grid_for(P, kWlThreads), bblocks = grid_for(B, kWlThreads);
    int64_t launches = 0, rounds = 0, props = 0, xrounds = 0, xprops = 0;
    bool more = false;
    if (P) {
        k_wl_init<<<pblocks, kWlThreads, 0, st>>>(n, d_forced);
        ++launches;
    }
    k_wl_max<<<bblocks, kWlThreads, 0, st>>>(B, n.load, n.ctl + U_PEAK0);
    ++launches;
    HIP_TRY(hipGetLastError());

    if (one) {
        if (P) {
            if (exchange) k_wl_one<true><<<1, kWlOneThreads, 3 * (size_t)B * sizeof(u64), st>>>(x, max_rounds);
            else k_wl_one<false><<<1, kWlOneThreads, 3 * (size_t)B * sizeof(u64), st>>>(n, max_rounds);
            ++launches;
            HIP_TRY(hipGetLastError());
        }
    } else if (P) {   // two launches per round; with exchange three: its propose sees the round's move count and steps aside, the apply does either kind
        uint32_t cnt[2 * kWlBatch] = {};   // the second row stays 0 without exchange
        const auto propose = [&](int r, int i) {   // round r, counted in column i
            k_wl_propose<<<pblocks, kWlThreads, 0, st>>>(n, r, d_cnt + i);
            if (exchange) k_wlx_propose<<<pblocks, kWlThreads, 0, st>>>(x, r, d_cnt + i, d_cnt + kWlBatch + i);
            launches += exchange ? 2 : 1;
        };
        for (int r = 0, done = 0; !done;) {
            if (r >= kWlHardRounds) return fail(KAO_ERR_HIP, fn + "the rounds did not finish");
            const int nb = max_rounds > 0 ? std::min(kWlBatch, max_rounds - r) : kWlBatch;
            HIP_TRY(hipMemsetAsync(d_cnt, 0, ncnt * sizeof(uint32_t), st));
            if (nb == 0) propose(r, 0);   // max_rounds rounds have run, every one with a proposal: is there more to do?
            for (int i = 0; i < nb; ++i) {
                propose(r + i, i);
                if (exchange) k_wl_apply<true><<<pblocks, kWlThreads, 0, st>>>(x, r + i, d_cnt + i);
                else k_wl_apply<false><<<pblocks, kWlThreads, 0, st>>>(n, r + i, nullptr);
                ++launches;
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(cnt, d_cnt, ncnt * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (nb == 0) { more = cnt[0] != 0 || cnt[kWlBatch] != 0; break; }
            for (int i = 0; i < nb && !done; ++i) {   // the first round with no proposal of either kind ends the call; the ones after it changed nothing
                const uint32_t cm = cnt[i], cx = cnt[kWlBatch + i];
                if (cm == 0 && cx == 0) done = 1;
                else {
                    ++rounds; props += cm + cx;
                    if (cm == 0) { ++xrounds; xprops += cx; }
                }
            }
            r += nb;
        }
    }

    k_wl_rank<<<bblocks, kWlThreads, 0, st>>>(B, n.load, d_rank, n.ctl + U_PEAK1);
    ++launches;
    if (P) {
        k_wl_finish<<<pblocks, kWlThreads, 0, st>>>(n, d_rank, d_hist, d_led, d_rows, dry_run);
        ++launches;
    }
    k_wl_scan<<<1, kWlThreads, 0, st>>>(B, d_hist, d_forced, d_led, n.ctl);
    ++launches;
    HIP_TRY(hipGetLastError());
    u64 ctl[U_N];
    HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    if (P && !dry_run) HIP_TRY(hipMemcpyAsync(rows, d_rows, (size_t)PW * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (one) {
        rounds = (int64_t)ctl[U_ROUNDS]; props = (int64_t)ctl[U_PROPS]; more = ctl[U_MORE] != 0;
        xrounds = (int64_t)ctl[U_XROUNDS]; xprops = (int64_t)ctl[U_XPROPS];
    }
    if (rounds >= kWlHardRounds) return fail(KAO_ERR_HIP, fn + "the rounds did not finish");
    const uint64_t lb = std::max({(uint64_t)ctl[U_MAXW], (uint64_t)ctl[U_FORCED], (uint64_t)ctl[U_LEVEL]});
    *n_changed = (int32_t)ctl[U_CHANGED];
    *peak_before = ctl[U_PEAK0];
    *peak_after = ctl[U_PEAK1];
    *lower_bound = lb;
    *status = ctl[U_PEAK1] == lb ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
    if (stats) {
        stats[0] = rounds; stats[1] = (int64_t)(ctl[U_MOVES] + ctl[U_XCH]); stats[2] = props; stats[3] = launches; stats[4] = one ? 1 : 0;
        stats[5] = more ? 1 : 0; stats[6] = ctl[U_LEVEL] == lb ? (int64_t)ctl[U_LEVELK] : 0; stats[7] = (int64_t)ctl[U_LEADING];
        if (exchange) { stats[8] = xrounds; stats[9] = (int64_t)ctl[U_XCH]; stats[10] = xprops; stats[11] = (int64_t)ix.ent.size(); }
    }
    return KAO_OK;
}

}  // namespace

extern "C" int kao_wleaders_test_path(int32_t path) {
    if (path < 0 || path > 2) return fail(KAO_ERR_INVALID, "kao_wleaders_test_path: path outside 0..2");
    const int was = t_wl_path;
    t_wl_path = path;
    return was;
}

extern "C" int64_t kao_wleaders_last_setup_us(void) { return t_wlx_setup_us; }

extern "C" int kao_balance_leaders_weighted(int32_t n_brokers, int32_t n_partitions, int32_t width, uint16_t *rows, const uint64_t *weight,
                                            uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_changed, uint64_t *peak_before,
                                            uint64_t *peak_after, uint64_t *lower_bound, int32_t *status, int64_t stats[8]) {
    return wl_call(false, "kao_balance_leaders_weighted: ", n_brokers, n_partitions, width, rows, weight, min_gain, max_rounds, dry_run, n_changed,
                   peak_before, peak_after, lower_bound, status, stats);
}

extern "C" int kao_balance_leaders_weighted_exchange(int32_t n_brokers, int32_t n_partitions, int32_t width, uint16_t *rows, const uint64_t *weight,
                                                     uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_changed,
                                                     uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound, int32_t *status,
                                                     int64_t stats[12]) {
    return wl_call(true, "kao_balance_leaders_weighted_exchange: ", n_brokers, n_partitions, width, rows, weight, min_gain, max_rounds, dry_run,
                   n_changed, peak_before, peak_after, lower_bound, status, stats);
}
