// kao_eval.hip -- K-eval (gfx950) and the two small kernels around it, with their launchers.
//   k_eval         : full evaluation (objective README.md:145-146 and rows C1..C7 README.md:148-180) of complete compact candidates
//                    streamed from HBM, one wavefront per candidate, ending in the wavefront -> workgroup -> atomicMin reduce of the
//                    packed (violation, cost, id) key.
//   k_gather       : every topic's winner -> contiguous read-back buffers.
//   k_adopt_global : adopt the best keys that arrived from other GPUs.
// Integer-only, wave64.  Of kao_search_dev.h only band() is used.
#include "kao_search_dev.h"

namespace kao {

// ------------------------------------------------------------------------------------------------
// K-eval
// ------------------------------------------------------------------------------------------------
// NE = replica slots handled per partition: 4 (RF and current RF <= 4) or 8.
// kCoop = false: one wavefront per candidate (4 candidates in flight per workgroup) -- batches that fill the device.
// kCoop = true : the WHOLE workgroup evaluates one candidate, its four wavefronts striding the partitions over one shared set
//                of LDS counters -- few large candidates (a 30,000-partition topic has 256 restarts; KAO-CX scores <= 513
//                realisations): one wavefront per candidate left 3 of 4 SIMDs idle and took 469 dependent trips per candidate.
//                All sums are integers, so the split changes no result.
// RFT > 0 (round 6): every topic of the launch has replication factor RFT -- the slot loops run RFT times without the `k >= RF` guards and the
//                C7 compare square is RFT x RFT instead of NE x NE (RF 3 in four slots: 9 of 16); RFT = 0: RF is read per topic.
template <int NE, bool kCoop, int RFT = 0>
__global__ __launch_bounds__(256) void k_eval(EvalPools pl) {
    constexpr int RFE = RFT ? RFT : NE;      // slots the loops visit
    constexpr bool kLds = RFT > 0;           // the RF-uniform instantiation is launched only with the current assignment staged in LDS (launch_eval)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_all[];
    unsigned long long *wave_key = reinterpret_cast<unsigned long long *>(smem_all);  // [kWaves], 32 B
    unsigned char *smem = smem_all + 32;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int4 bm = pl.block_map[blockIdx.x];
    const TopicDev *TD = pl.topics + bm.x;
    const int B = TD->B, R = TD->R, P = TD->P, RF = RFT ? RFT : TD->RF, rf_cur = TD->rf_cur;
    const int rep_lo = TD->rep_lo, rep_hi = TD->rep_hi, lead_lo = TD->lead_lo, lead_hi = TD->lead_hi;
    const int rack_lo = TD->rack_lo, rack_hi = TD->rack_hi, prack_lo = TD->prack_lo, prack_hi = TD->prack_hi;
    const int w00 = TD->w00, w01 = TD->w01, w10 = TD->w10, w11 = TD->w11;
    const bool cur_lds = kLds || pl.cur_in_lds != 0;
    // C7 of a partition whose three replicas sit on one / two / three racks (RFT == 3)
    const int c7_one = band(3, prack_lo, prack_hi) + (R - 1) * prack_lo;
    const int c7_two = band(2, prack_lo, prack_hi) + band(1, prack_lo, prack_hi) + (R - 2) * prack_lo;
    const int c7_three = 3 * band(1, prack_lo, prack_hi) + (R - 3) * prack_lo;

    // ---- LDS carve: [wave_key 32 B] [RACK u8[maxB~]] [CURD u16[maxP][NE]] then per wave [C u32[maxB~]] [K int[256]]
    const int r_bytes = (pl.maxB + 15) & ~15;
    const int d_bytes = cur_lds ? pl.maxP * NE * 2 : 0;  // huge topics read the current assignment from global memory
    const int c_bytes = (pl.maxB * 4 + 15) & ~15;
    uint8_t *RACK = smem;
    uint16_t *CURD = reinterpret_cast<uint16_t *>(smem + r_bytes);
    unsigned char *wb = smem + r_bytes + ((d_bytes + 15) & ~15) + (kCoop ? 0 : wave) * (c_bytes + kRackTab * 4);
    int *red = reinterpret_cast<int *>(smem + r_bytes + ((d_bytes + 15) & ~15) + kWaves * (c_bytes + kRackTab * 4));   // [kWaves][8] (kCoop)
    const int tid = kCoop ? (int)threadIdx.x : lane, tstride = kCoop ? 256 : 64;
    uint32_t *C = reinterpret_cast<uint32_t *>(wb);
    int *K = reinterpret_cast<int *>(wb + c_bytes);

    // ---- stage the broker->rack table and the current assignment (padded to NE slots with 0xFFFF) ----
    for (int b = threadIdx.x; b < B; b += 256) RACK[b] = pl.rackof_pool[TD->rackof_off + b];
    const uint16_t *curd = pl.curd_pool + TD->curd_off;
    const uint32_t *bwd = TD->has_bw ? pl.bwd_pool + TD->bwd_off : nullptr;   // broker weights, dense index (global memory / L2)
    if (cur_lds)
        for (int i = threadIdx.x; i < P * NE; i += 256) {
            const int p = i / NE, k = i - p * NE;
            CURD[i] = k < rf_cur ? curd[(size_t)p * rf_cur + k] : (uint16_t)0xFFFFu;
        }
    __syncthreads();

    unsigned long long my_key = ~0ull;
    const int nB4 = (B + 3) >> 2;  // counters zeroed 16 bytes per lane per store (C is 16-byte aligned and padded)
    // Rack counters: the 64 lanes of a wavefront hit only R addresses, so one LDS atomic per replica would serialise (10 racks:
    // ~5 lanes per address).  They are privatised per 16-lane row -- 4 copies inside the same 256-entry table when R <= 64 --
    // added without return value, and the band rows C6 are evaluated from the totals in one pass at the end.
    const int KR = (R + 15) & ~15;
    const int kcopy = 4 * KR <= kRackTab ? (lane >> 4) * KR : 0;
    const bool k4 = 4 * KR <= kRackTab;
    const bool big = !kLds && P * RF > 65535;   // only then can a 16-bit per-broker counter overflow (the RF-3 instantiation runs with the current assignment in LDS: at most 20,480 partitions x 3)
    for (int ci = bm.y + (kCoop ? 0 : wave); ci < bm.y + bm.z; ci += (kCoop ? 1 : kWaves)) {
        const uint16_t *cand = pl.cand + TD->best_off + (uint64_t)ci * P * RF;
        for (int b4 = tid; b4 < nB4; b4 += tstride) reinterpret_cast<uint4 *>(C)[b4] = make_uint4(0, 0, 0, 0);
        for (int r = tid; r < (k4 ? 4 * KR : KR); r += tstride) K[r] = 0;      // (only the entries the atomics below and the C6 pass touch)
        if (kCoop) __syncthreads();
        // Broker band violations are accumulated from the value each LDS atomic RETURNS: adding a replica to a
        // broker whose count was c changes band(c) by (c >= hi) - (c < lo), and sum_b band(0) = B*lo, so
        // no pass over all brokers is needed.  Packed partial sums: low half = #(old >= hi), high = #(old < lo).
        int obj = 0;
        uint32_t s12 = 0;  // v1 | v2 << 16
        // C3 / C4 are COUNTS of lanes (old count at or above the upper end, below the lower end): each is a compare into a scalar pair and a
        // population count, accumulated in scalar registers -- no per-lane sum, no wavefront reduction (round 6, last: they were two of the six
        // words of wave_sum6 and five vector instructions per slot)
        int n3hi = 0, n3lo = 0, n4hi = 0, n4lo = 0;
        uint32_t s57 = 0;  // v5 | v7 << 16
        bool ovf = false;
        for (int p = tid; p < P; p += tstride) {
            const uint16_t *ap = cand + (size_t)p * RF;  // a wavefront reads 64*RF consecutive u16: coalesced
            uint32_t bk[NE], rk[NE], ck[NE];
            uint32_t cw[NE / 2];   // the partition's current replicas, two u16 per word: one ds_read_b64 / b128 when staged in LDS
            if (cur_lds) {
                if (NE == 4) { const uint2 v = reinterpret_cast<const uint2 *>(CURD)[p]; cw[0] = v.x; cw[1] = v.y; }
                else { const uint4 v = reinterpret_cast<const uint4 *>(CURD)[p]; cw[0] = v.x; cw[1] = v.y; cw[2 % (NE / 2)] = v.z; cw[3 % (NE / 2)] = v.w; }
            }
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                bk[k] = k < RF ? (uint32_t)ap[k < RF ? k : 0] : 0xFFFFu;
                rk[k] = 0xFFu;
                ck[k] = cur_lds ? ((k & 1) ? cw[k >> 1] >> 16 : cw[k >> 1] & 0xFFFFu)
                                      : (k < rf_cur ? (uint32_t)curd[(size_t)p * rf_cur + (k < rf_cur ? k : 0)] : 0xFFFFu);
            }
            int missing = 0;
            // One slot of the trip (KAO_EVAL_SLOT).  VALID is the lane's own "this slot holds a broker", or the literal true when every lane of
            // the trip has one (the usual case, tested once per trip with a ballot): the body then has no per-lane branch and the counts sit in
            // wave-uniform control flow.  Otherwise the counts are taken where the lanes have met again -- the scalar accumulators live in every
            // lane's copy of the loop state, and a lane that sat out a slot would miss its counts (lane 0, whose copy is read in the end, is in
            // every trip: partitions ascend with the lane).
#define KAO_EVAL_SLOT(VALID) do { \
                uint32_t oc = 0; \
                if (!(VALID)) ++missing; \
                else { \
                    rk[k] = RACK[b]; \
                    oc = atomicAdd(&C[b], k == 0 ? 0x10001u : 1u); \
                    __hip_atomic_fetch_add(&K[kcopy + rk[k]], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
                    if (big) ovf |= (oc & 0xFFFFu) == 0xFFFFu; \
                    bool fol = false, dup = false; \
                    _Pragma("unroll") for (int j = 1; j < NE; ++j) fol |= ck[j] == b; \
                    _Pragma("unroll") for (int j = 0; j < k; ++j) dup |= bk[j] == b; \
                    obj += (ck[0] == b) ? (k == 0 ? w00 : w01) : (fol ? (k == 0 ? w10 : w11) : 0); \
                    if (bwd) { const uint32_t bw = bwd[b]; obj += (int)(bw & 0xFFFFu) + (k == 0 ? (int)(bw >> 16) : 0); } \
                    s57 += (uint32_t)dup;  /* C5: f+l <= 1 (an earlier slot holds the same broker) */ \
                } \
                const int cr = (int)(oc & 0xFFFFu); \
                n3hi += wave_count((VALID) & (cr >= rep_hi)); n3lo += wave_count((VALID) & (cr < rep_lo));         /* C3 */ \
                if (k == 0) { \
                    const int cl = (int)(oc >> 16); \
                    n4hi += wave_count((VALID) & (cl >= lead_hi)); n4lo += wave_count((VALID) & (cl < lead_lo));   /* C4 */ \
                } \
            } while (0)
            bool any_empty = false;
#pragma unroll
            for (int k = 0; k < RFE; ++k) {
                if (!RFT && k >= RF) break;
                any_empty |= bk[k] >= (uint32_t)B;
            }
            const bool trip_full = __ballot(any_empty) == 0ull;      // wave-uniform: no lane of this trip has an empty / out-of-range slot
            if (trip_full) {
#pragma unroll
                for (int k = 0; k < RFE; ++k) {
                    if (!RFT && k >= RF) break;
                    const uint32_t b = bk[k];
                    KAO_EVAL_SLOT(true);
                }
            } else {
#pragma unroll
                for (int k = 0; k < RFE; ++k) {
                    if (!RFT && k >= RF) break;
                    const uint32_t b = bk[k];
                    const bool valid = b < (uint32_t)B;
                    KAO_EVAL_SLOT(valid);
                }
            }
#undef KAO_EVAL_SLOT
            s12 += (uint32_t)missing + ((uint32_t)(bk[0] >= (uint32_t)B) << 16);  // C1: sum_b (f+l) = RF ; C2: exactly one leader
            // C7: replicas per partition per rack, over all R racks (each rack counted at its first slot)
            if (RFT == 3 && trip_full) {
                // three filled slots (no lane of this trip has an empty one: wave-uniform) fall on one, two or three racks -- the row's value
                // in each case is a constant of the topic (c7_one / c7_two / c7_three: the sums the general loop below would form)
                const bool e01 = rk[0] == rk[1], e02 = rk[0] == rk[2], e12 = rk[1] == rk[2];
                s57 += (uint32_t)((e01 & e12) ? c7_one : ((e01 | e02 | e12) ? c7_two : c7_three)) << 16;
            } else {
                int touched = 0, s7 = 0;
#pragma unroll
                for (int k = 0; k < RFE; ++k) {
                    bool first = rk[k] != 0xFFu;
                    int cnt = 0;
#pragma unroll
                    for (int j = 0; j < RFE; ++j) { cnt += (int)(rk[j] == rk[k]); if (j < k) first &= rk[j] != rk[k]; }
                    if (first) { s7 += band(cnt, prack_lo, prack_hi); touched++; }
                }
                s57 += (uint32_t)(s7 + (R - touched) * prack_lo) << 16;
            }
        }
        // C6 from the rack totals (the wavefront's own LDS operations complete in order: no barrier needed; the cooperating
        // wavefronts of kCoop meet at one)
        if (kCoop) __syncthreads();
        int s6 = 0;
        for (int r = tid; r < R; r += tstride) {
            const int tot = k4 ? K[r] + K[KR + r] + K[2 * KR + r] + K[3 * KR + r] : K[r];
            s6 += band(tot, rack_lo, rack_hi);
        }
        if (big && __ballot(ovf) != 0ull && pl.overflow && lane == 0) atomicOr(pl.overflow, 1);
        int v1, v2, v3, v4, v5, v6, v7;   // (v3, v4 without their constants B * lo until the partial sums have met)
        v3 = __builtin_amdgcn_readfirstlane(n3hi - n3lo); v4 = __builtin_amdgcn_readfirstlane(n4hi - n4lo);      // lane 0's copy (see above): wave-uniform from here on
        if (P * RF <= 32767) {  // packed halves cannot carry: every count is at most P*RF -- the four words are summed in one go (wave_sum4)
            int t[4] = {obj, (int)s12, (int)s57, s6};
            wave_sum4(t);
            const uint32_t t12 = (uint32_t)t[1], t57 = (uint32_t)t[2];
            obj = t[0]; v6 = t[3];
            v1 = (int)(t12 & 0xFFFFu); v2 = (int)(t12 >> 16);
            v5 = (int)(t57 & 0xFFFFu); v7 = (int)(t57 >> 16);
        } else {  // huge topic: per-lane halves still fit 16 bits, the wavefront totals do not -> sum them unpacked
            obj = wave_sum(obj);
            v1 = wave_sum((int)(s12 & 0xFFFFu)); v2 = wave_sum((int)(s12 >> 16));
            v5 = wave_sum((int)(s57 & 0xFFFFu)); v7 = wave_sum((int)(s57 >> 16));
            v6 = wave_sum(s6);
        }
        if (kCoop) {   // the four wavefronts' partial sums meet in LDS; every wavefront reads the totals
            if (lane == 0) { int *q = red + wave * 8; q[0] = obj; q[1] = v1; q[2] = v2; q[3] = v3; q[4] = v4; q[5] = v5; q[6] = v6; q[7] = v7; }
            __syncthreads();
            obj = v1 = v2 = v3 = v4 = v5 = v6 = v7 = 0;
            for (int w = 0; w < kWaves; ++w) {
                const int *q = red + w * 8;
                obj += q[0]; v1 += q[1]; v2 += q[2]; v3 += q[3]; v4 += q[4]; v5 += q[5]; v6 += q[6]; v7 += q[7];
            }
            __syncthreads();   // the counters and `red` are reused by the next candidate
        }
        v3 += B * rep_lo; v4 += B * lead_lo;
        const int v0 = v1 + v2 + v3 + v4 + v5 + v6 + v7;
        const int out = bm.w + (ci - bm.y);
        if (lane == 0 && (!kCoop || wave == 0)) {
            if (pl.objective) pl.objective[out] = obj;
            if (pl.violations) {
                int4 *vo = reinterpret_cast<int4 *>(pl.violations + (size_t)out * 8);
                vo[0] = make_int4(v0, v1, v2, v3);
                vo[1] = make_int4(v4, v5, v6, v7);
            }
        }
        const unsigned long long key = ((unsigned long long)min(v0, 0xFFFFF) << 44) |
                                       ((unsigned long long)(kObjCap - (uint32_t)min(obj, (int)kObjCap)) << 20) |
                                       (unsigned long long)(ci & 0xFFFFF);
        my_key = key < my_key ? key : my_key;
    }
    if (pl.best_key) {  // workgroup reduce of the wave-uniform keys, one atomicMin per workgroup per topic
        if (lane == 0) wave_key[wave] = my_key;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long k = wave_key[0];
            for (int w = 1; w < kWaves; ++w) k = wave_key[w] < k ? wave_key[w] : k;
            if (k != ~0ull) atomicMin(pl.best_key + bm.x, k);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K-gather: winners -> contiguous read-back buffers
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_gather(const TopicDev *topics, const unsigned long long *keys, const uint16_t *best_pool,
                                               const int32_t *viol, uint16_t *win_assign, int32_t *win_viol) {
    const TopicDev *TD = topics + blockIdx.x;
    const unsigned long long key = keys[blockIdx.x];
    if (key == ~0ull) return;
    const int rho = (int)(key & 0xFFFFFull);
    if (rho == (int)kExternalRestart) {  // the topic's best came from another GPU (kao_solve_multi): win_assign already holds it
        if (threadIdx.x < 8) win_viol[blockIdx.x * 8 + threadIdx.x] = 0;  // only feasible assignments are exchanged
        return;
    }
    const int n = TD->P * TD->RF;
    const uint16_t *src = best_pool + TD->best_off + (uint64_t)rho * n;
    uint16_t *dst = win_assign + TD->win_off;
    for (int i = threadIdx.x; i < n; i += 64) dst[i] = src[i];
    if (threadIdx.x < 8) win_viol[blockIdx.x * 8 + threadIdx.x] = viol[(size_t)(TD->restart_base + rho) * 8 + threadIdx.x];
}

// After the min-allreduce of the packed best keys across GPUs (kao_solve_multi, replicated topics): where another GPU's key
// beats the local one, adopt it with the reserved restart id kExternalRestart (its assignment arrives by broadcast).
__global__ __launch_bounds__(64) void k_adopt_global(unsigned long long *keys, const unsigned long long *glob, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long g = glob[i];
    if (g < keys[i] && (g >> 44) == 0) keys[i] = g | (unsigned long long)kExternalRestart;
}

// ------------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------------
// the "LDS carve" of k_eval, summed (pinned below): wave_key, RACK, CURD (only with the current assignment in LDS), kWaves x (C, K), red
constexpr size_t eval_lds_total(size_t maxP, size_t maxB, bool cur_in_lds, size_t ne) {
    const size_t r = (maxB + 15) & ~(size_t)15, d = cur_in_lds ? (maxP * 2 * ne + 15) & ~(size_t)15 : 0;
    const size_t c = (maxB * 4 + 15) & ~(size_t)15;
    return 32 + r + d + kWaves * (c + kRackTab * 4) + kWaves * 8 * 4;   // (+ the partial sums of the cooperative mode)
}
size_t eval_lds_bytes(int maxP, int maxB, bool cur_in_lds, int ne) { return eval_lds_total((size_t)maxP, (size_t)maxB, cur_in_lds, (size_t)ne); }
static_assert(eval_lds_total(50, 500, true, 4) == 13168 && eval_lds_total(50, 500, false, 4) == 12768, "eval_lds_total no longer sums the LDS carve of k_eval");   // config 4, current assignment in LDS / in global memory

void launch_eval(const EvalPools &pools, int n_blocks, int ne, void *stream) {
    const size_t lds = eval_lds_bytes(pools.maxP, pools.maxB, pools.cur_in_lds != 0, ne);
    hipStream_t st = static_cast<hipStream_t>(stream);
    with_flags(ne == 8, pools.coop != 0, [&](auto k8, auto coop) {
        constexpr int NE = decltype(k8)::value ? 8 : 4;
        constexpr bool kCoop = decltype(coop)::value;
        if constexpr (NE == 4 && !kCoop)   // RF 3 throughout and the current assignment in LDS: the instantiation without slot guards
            if (pools.rf_uniform == 3 && pools.cur_in_lds) return launch_lds<k_eval<4, false, 3>>(dim3(n_blocks), dim3(256), lds, st, pools);
        launch_lds<k_eval<NE, kCoop>>(dim3(n_blocks), dim3(256), lds, st, pools);
    });
}

void launch_gather(const TopicDev *topics, int n_topics, const unsigned long long *keys, const uint16_t *best_pool,
                   const int32_t *viol, uint16_t *win_assign, int32_t *win_viol, void *stream) {
    hipLaunchKernelGGL(k_gather, dim3(n_topics), dim3(64), 0, static_cast<hipStream_t>(stream), topics, keys, best_pool, viol,
                       win_assign, win_viol);
}

void launch_adopt_global(unsigned long long *keys, const unsigned long long *glob, int n, void *stream) {
    hipLaunchKernelGGL(k_adopt_global, dim3((n + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), keys, glob, n);
}

}  // namespace kao
