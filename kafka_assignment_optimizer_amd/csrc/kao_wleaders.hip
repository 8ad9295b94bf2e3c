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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "kao_host.h"
#include "kao_plan_dev.h"   // DESCENT_KEY, descent_gains, descent_bid, lane_count_to, swap_leader

namespace {

constexpr int kWlThreads = 256;
constexpr int kWlBatch = 32;            // rounds enqueued between two reads of the proposal counts
constexpr int kWlOneThreads = 1024;     // the single workgroup
constexpr int kWlOneMaxB = 2048;        // ... holds loads + two minkey rows in LDS: 24 bytes per broker, 48 KiB
constexpr int kWlOneMaxP = 4096;        // ... and is chosen up to this many partitions (threshold)
constexpr int kWlHardRounds = 1 << 26;  // no descent gets here; a guard against an endless loop
constexpr u64 kWlNoKey = ~0ull;
enum { U_PEAK0 = 0, U_PEAK1, U_MOVES, U_PROPS, U_ROUNDS, U_MAXW, U_FORCED, U_LEVEL, U_LEVELK, U_CHANGED, U_LEADING, U_MORE, U_N = 16 };

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

__device__ inline void wl_max_to(u64 v, u64 *dst) {   // all 64 lanes active
    for (int off = 32; off > 0; off >>= 1) v = max(v, (u64)__shfl_xor((long long)v, off));
    if (__lane_id() == 0 && v > 0) atomicMax(dst, v);
}

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
    wl_max_to(w, &n.ctl[U_MAXW]);
}

__global__ void k_wl_max(int B, const u64 *__restrict__ x, u64 *__restrict__ dst) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    wl_max_to(b < B ? x[b] : 0, dst);
}

// ---- a round on the multi-launch path -----------------------------------------------------------------------------------------------
__global__ void k_wl_propose(WlNet n, int r, uint32_t *__restrict__ count) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool prop = false;
    if (p < n.P) {
        int a = 0, b = 0, slot = 0;
        u64 key = kWlNoKey;
        prop = wl_propose(n, p, n.load, a, b, slot, key);
        n.key[p] = key;
        if (prop) {
            n.slot[p] = (uint8_t)slot;
            u64 *row = n.mk + (size_t)(r & 1) * n.B;
            descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&row[a], key);
            descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&row[b], key);
        }
    }
    lane_count_to(prop, count);
}

__global__ void k_wl_apply(WlNet n, int r) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    {   // the row of round r + 1 was last read by the apply of round r - 1
        u64 *clr = n.mk + (size_t)((r + 1) & 1) * n.B;
        for (int e = p; e < n.B; e += gridDim.x * blockDim.x) clr[e] = kWlNoKey;
    }
    bool won = false;
    if (p < n.P) {
        const u64 key = n.key[p];
        if (key != kWlNoKey) {
            const uint16_t *row = n.rows + (size_t)p * n.W;
            const int slot = n.slot[p], a = row[n.lead[p]], b = row[slot];
            const u64 *mine = n.mk + (size_t)(r & 1) * n.B;
            won = mine[a] == key && mine[b] == key;
            if (won) {   // no other winner touches a or b
                const u64 w = n.weight[p];
                n.load[a] -= w;
                n.load[b] += w;
                n.lead[p] = (uint8_t)slot;
            }
        }
    }
    lane_count_to(won, &n.ctl[U_MOVES]);
}

// ---- every round in one launch: one workgroup, loads and minkey rows in LDS ---------------------------------------------------------
__global__ __launch_bounds__(kWlOneThreads) void k_wl_one(WlNet n, int max_rounds) {
    extern __shared__ u64 wl_lds[];
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
    for (int r = 0; r < kWlHardRounds; ++r) {
        u64 *row = mk + (size_t)(r & 1) * n.B, *other = mk + (size_t)((r + 1) & 1) * n.B;
        int mine = 0;
        for (int p = tid; p < n.P; p += kWlOneThreads) {
            int a = 0, b = 0, slot = 0;
            u64 key = kWlNoKey;
            const bool prop = wl_propose(n, p, load, a, b, slot, key);
            n.key[p] = key;   // read back by this thread alone
            if (prop) {
                n.slot[p] = (uint8_t)slot;
                atomicMin(&row[a], key);
                atomicMin(&row[b], key);
                ++mine;
            }
        }
        if (!__syncthreads_or(mine)) break;
        if (max_rounds > 0 && r >= max_rounds) { more = 1; break; }
        ++rounds;
        props += (u64)mine;
        for (int p = tid; p < n.P; p += kWlOneThreads) {
            const u64 key = n.key[p];
            if (key == kWlNoKey) continue;
            const uint16_t *rw = n.rows + (size_t)p * n.W;
            const int slot = n.slot[p], a = rw[n.lead[p]], b = rw[slot];
            if (row[a] == key && row[b] == key) {
                const u64 w = n.weight[p];
                load[a] -= w;
                load[b] += w;
                n.lead[p] = (uint8_t)slot;
                ++moves;
            }
        }
        for (int b = tid; b < n.B; b += kWlOneThreads) other[b] = kWlNoKey;
        __syncthreads();
    }
    __syncthreads();
    for (int b = tid; b < n.B; b += kWlOneThreads) n.load[b] = load[b];
    if (props) atomicAdd(&n.ctl[U_PROPS], props);
    if (moves) atomicAdd(&n.ctl[U_MOVES], moves);
    if (tid == 0) {
        n.ctl[U_ROUNDS] = (u64)rounds;
        n.ctl[U_MORE] = (u64)more;
    }
}

// ---- the certificate and the result -------------------------------------------------------------------------------------------------
// (rank, histogram and scan in three launches over all brokers; k_wfo_solve of kao_wfailover.hip ranks a compacted set inside its
// workgroup and reuses its LDS for the histogram: not shared)
// rank[b] = brokers ahead of b by (load descending, index ascending); the peak on the way
__global__ __launch_bounds__(kWlThreads) void k_wl_rank(int B, const u64 *__restrict__ load, int32_t *__restrict__ rank, u64 *__restrict__ peak) {
    __shared__ u64 tile[kWlThreads];
    const int b = blockIdx.x * kWlThreads + threadIdx.x;
    const u64 mine = b < B ? load[b] : 0;
    int r = 0;
    for (int base = 0; base < B; base += kWlThreads) {
        const int cnt = min(kWlThreads, B - base);
        if ((int)threadIdx.x < cnt) tile[threadIdx.x] = load[base + threadIdx.x];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const u64 x = tile[j];
            r += (x > mine || (x == mine && base + j < b)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (b < B) rank[b] = r;
    wl_max_to(mine, peak);
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

int validate_weighted(int32_t B, int32_t P, int32_t W, const uint16_t *rows, const uint64_t *weight, const int32_t *n_changed,
                      const uint64_t *peak_before, const uint64_t *peak_after, const uint64_t *lower_bound, const int32_t *status) {
    const std::string fn = "kao_balance_leaders_weighted: ";
    if (!rows || !weight || !n_changed || !peak_before || !peak_after || !lower_bound || !status) return fail(KAO_ERR_INVALID, fn + "null pointer");
    int rc = check_dims(fn, B, P, W);
    if (!rc) rc = check_slot_cap(fn, P, W);
    if (!rc) rc = check_rows(fn, B, P, W, rows);
    return rc ? rc : check_weight_sum(fn, P, weight);
}

}  // namespace

extern "C" int kao_wleaders_test_path(int32_t path) {
    if (path < 0 || path > 2) return fail(KAO_ERR_INVALID, "kao_wleaders_test_path: path outside 0..2");
    const int was = t_wl_path;
    t_wl_path = path;
    return was;
}

extern "C" int kao_balance_leaders_weighted(int32_t n_brokers, int32_t n_partitions, int32_t width, uint16_t *rows, const uint64_t *weight,
                                            uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_changed, uint64_t *peak_before,
                                            uint64_t *peak_after, uint64_t *lower_bound, int32_t *status, int64_t stats[8]) {
    int rc = validate_weighted(n_brokers, n_partitions, width, rows, weight, n_changed, peak_before, peak_after, lower_bound, status);
    if (rc) return rc;
    if ((rc = require_init())) return rc;
    const int B = n_brokers, P = n_partitions, W = width, PW = P * W;
    const bool one = t_wl_path == 1 || (t_wl_path == 0 && B <= kWlOneMaxB && P <= kWlOneMaxP);
    if (one && B > kWlOneMaxB) return fail(KAO_ERR_UNSUPPORTED, "kao_balance_leaders_weighted: the single-workgroup path holds at most " + std::to_string(kWlOneMaxB) + " brokers");

    // one arena: ctl u64[U_N] | count u32[kWlBatch] | load, forced, hist u64[B] | led, rank i32[B] (zeroed up to here) | mk u64[2B]
    //            (all ones) | key, weight u64[P] | rows u16[PW] | lead, slot u8[P]
    Carve cv;
    const size_t o_ctl = cv.take<u64>(U_N), o_cnt = cv.take<uint32_t>(kWlBatch), o_load = cv.take<u64>(B), o_forced = cv.take<u64>(B),
                 o_hist = cv.take<u64>(B), o_led = cv.take<int32_t>(B), o_rank = cv.take<int32_t>(B), zeroed = cv.end(),
                 o_mk = cv.take<u64>(2 * (size_t)B), o_key = cv.take<u64>(P), o_w = cv.take<u64>(P), o_rows = cv.take<uint16_t>(PW),
                 o_lead = cv.take<uint8_t>(P), o_slot = cv.take<uint8_t>(P);
    CallBufs m;
    if ((rc = m.open(cv.end()))) return rc;
    hipStream_t st = m.stream;
    uint16_t *d_rows = m.at<uint16_t>(o_rows);
    uint32_t *d_cnt = m.at<uint32_t>(o_cnt);
    int32_t *d_led = m.at<int32_t>(o_led), *d_rank = m.at<int32_t>(o_rank);
    u64 *d_forced = m.at<u64>(o_forced), *d_hist = m.at<u64>(o_hist);
    WlNet n;
    n.P = P; n.W = W; n.B = B; n.min_gain = min_gain;
    n.rows = d_rows; n.weight = m.at<u64>(o_w); n.lead = m.at<uint8_t>(o_lead); n.slot = m.at<uint8_t>(o_slot); n.key = m.at<u64>(o_key);
    n.load = m.at<u64>(o_load); n.mk = m.at<u64>(o_mk); n.ctl = m.at<u64>(o_ctl);

    HIP_TRY(hipMemsetAsync(m.arena, 0, zeroed, st));
    HIP_TRY(hipMemsetAsync(n.mk, 0xFF, 2 * (size_t)B * sizeof(u64), st));
    if (P) {
        HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<u64>(o_w), weight, (size_t)P * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    const unsigned pblocks = grid_for(P, kWlThreads), bblocks = grid_for(B, kWlThreads);
    int64_t launches = 0, rounds = 0, props = 0;
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
            k_wl_one<<<1, kWlOneThreads, 3 * (size_t)B * sizeof(u64), st>>>(n, max_rounds);
            ++launches;
            HIP_TRY(hipGetLastError());
        }
    } else if (P) {
        uint32_t cnt[kWlBatch];
        for (int r = 0, done = 0; !done;) {
            if (r >= kWlHardRounds) return fail(KAO_ERR_HIP, "kao_balance_leaders_weighted: the rounds did not finish");
            const int nb = max_rounds > 0 ? std::min(kWlBatch, max_rounds - r) : kWlBatch;
            HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof cnt, st));
            if (nb == 0) {   // max_rounds rounds have run, every one with a move: is there more to do?
                k_wl_propose<<<pblocks, kWlThreads, 0, st>>>(n, r, d_cnt);
                ++launches;
            }
            for (int i = 0; i < nb; ++i) {
                k_wl_propose<<<pblocks, kWlThreads, 0, st>>>(n, r + i, d_cnt + i);
                k_wl_apply<<<pblocks, kWlThreads, 0, st>>>(n, r + i);
                launches += 2;
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (nb == 0) { more = cnt[0] != 0; break; }
            for (int i = 0; i < nb && !done; ++i) {   // the first round without a proposal ends the descent; the ones after it changed nothing
                if (cnt[i] == 0) done = 1;
                else { ++rounds; props += cnt[i]; }
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
    if (one) { rounds = (int64_t)ctl[U_ROUNDS]; props = (int64_t)ctl[U_PROPS]; more = ctl[U_MORE] != 0; }
    if (rounds >= kWlHardRounds) return fail(KAO_ERR_HIP, "kao_balance_leaders_weighted: the rounds did not finish");
    const uint64_t lb = std::max({(uint64_t)ctl[U_MAXW], (uint64_t)ctl[U_FORCED], (uint64_t)ctl[U_LEVEL]});
    *n_changed = (int32_t)ctl[U_CHANGED];
    *peak_before = ctl[U_PEAK0];
    *peak_after = ctl[U_PEAK1];
    *lower_bound = lb;
    *status = ctl[U_PEAK1] == lb ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
    if (stats) {
        stats[0] = rounds; stats[1] = (int64_t)ctl[U_MOVES]; stats[2] = props; stats[3] = launches; stats[4] = one ? 1 : 0;
        stats[5] = more ? 1 : 0; stats[6] = ctl[U_LEVEL] == lb ? (int64_t)ctl[U_LEVELK] : 0; stats[7] = (int64_t)ctl[U_LEADING];
    }
    return KAO_OK;
}
