// kao_plan_dev.h -- device code the one-shot planners share: the 64-bit keys of successive shortest paths (kao_leaders.hip,
// kao_leaders_cluster.hip; DESIGN.md sections 4h, 4j), the wavefront count, the leader swap, the offsets of buckets
// (kao_failover_dev.h, kao_logdirs.hip; sections 4i, 4o), the pieces of the weighted descent (kao_wleaders.hip, kao_wfailover.hip,
// kao_disk.hip, kao_logdirs.hip; sections 4k, 4l, 4m, 4o), and what the two descents over all brokers share (kao_wleaders.hip,
// kao_disk.hip; sections 4k, 4m, 4q): the wavefront maximum and sum into a control word and the all-pairs rank.  Everything sits in an
// unnamed namespace; the device functions are inlined into their callers, and the one kernel is a template that only the files that
// launch it instantiate.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kao_bytes_code.h"   // wave_bytes_code

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

// ---- flow keys: (distance + 2^30) << 32 | arcs on the path, minimised as one word -------------------------------------------------
constexpr u64 kFlowInf = ~0ull;
constexpr u64 kFlowSource = (u64)(1u << 30) << 32;   // distance 0, no arc
constexpr uint32_t kFlowNoPred = 0xFFFFFFFFu;

// key of the head of an arc of cost c whose tail has key ku
__device__ __forceinline__ u64 flow_step(u64 ku, int c) { return ku + ((u64)(long long)c << 32) + 1ull; }

// cost of moving a partition's leader from slot l to slot j: -1 back to slot 0, +1 away from it, 0 otherwise (all 0 in a probe)
__device__ __forceinline__ int flow_slot_cost(int j, int l, bool costed) { return !costed ? 0 : (j == 0 ? -1 : (l == 0 ? 1 : 0)); }

// the start of a phase at node v: the nodes with excess are the sources
__device__ __forceinline__ void flow_seed(int v, const int32_t *e, u64 *k0, u64 *k1, uint32_t *pred) {
    const u64 k = e[v] > 0 ? kFlowSource : kFlowInf;
    k0[v] = k;
    k1[v] = k;
    pred[v] = kFlowNoPred;
}

// ---- the lanes of a wavefront for which `one` holds, added to *dst by the lowest of them (all 64 lanes active) ---------------------
template <class T>
__device__ __forceinline__ void lane_count_to(bool one, T *dst) {
    const u64 m = __ballot(one);
    if (m != 0ull && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(dst, (T)__popcll(m));
}

// the maximum and the sum of v over a wavefront, into *dst by lane 0 unless it is 0 (all 64 lanes active)
__device__ inline void wave_max_to(u64 v, u64 *dst) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, (u64)__shfl_xor((long long)v, off));
    if (__lane_id() == 0 && v > 0) atomicMax(dst, v);
}

__device__ inline void wave_sum_to(u64 v, u64 *dst) {
    for (int off = 32; off > 0; off >>= 1) v += (u64)__shfl_xor((long long)v, off);
    if (__lane_id() == 0 && v > 0) atomicAdd(dst, v);
}

// the output row of a partition whose leader is slot l != 0: slot 0 and slot l swapped
__device__ __forceinline__ void swap_leader(uint16_t *row, int l) {
    const uint16_t a = row[0], b = row[l];
    row[0] = b;
    row[l] = a;
}

// ---- the offsets of n buckets (the scenarios of kao_failover_dev.h, the brokers of kao_logdirs.hip) from their sizes: start[i] = sum of
// cnt[0..i), fill[i] = 0; max_n[0] = the largest cnt and, with a second count array, max_n[1] = the largest cnt2; max_n points into the
// caller's control block, whose words are Word.  One workgroup of 1,024 lanes.
template <class Word>
__global__ __launch_bounds__(1024) void k_bucket_offsets(int n, const int32_t *__restrict__ cnt, const int32_t *__restrict__ cnt2, int32_t *__restrict__ start,
                                                          int32_t *__restrict__ fill, Word *__restrict__ max_n) {
    __shared__ int32_t part[1024];
    __shared__ int32_t mx, mx2;
    const int tid = threadIdx.x, NT = blockDim.x, per = (n + NT - 1) / NT, lo = min(tid * per, n), hi = min(lo + per, n);
    if (tid == 0) { mx = 0; mx2 = 0; }
    __syncthreads();
    int s = 0, m = 0, m2 = 0;
    for (int i = lo; i < hi; ++i) { s += cnt[i]; m = max(m, cnt[i]); }
    for (int i = lo; cnt2 && i < hi; ++i) m2 = max(m2, cnt2[i]);
    part[tid] = s;
    if (m) atomicMax(&mx, m);
    if (m2) atomicMax(&mx2, m2);
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < NT; ++i) { const int v = part[i]; part[i] = acc; acc += v; }
        max_n[0] = (Word)mx;
        if (cnt2) max_n[1] = (Word)mx2;
    }
    __syncthreads();
    s = part[tid];
    for (int i = lo; i < hi; ++i) { start[i] = s; fill[i] = 0; s += cnt[i]; }
}

// ---- the weighted descent ---------------------------------------------------------------------------------------------------------
// key of the proposal of partition p (weight w) whose source carries `load`: the heaviest source first, then the heaviest
// partition, then the lowest index
// (a macro: as a function it changes the operand order of the kernels' v_or3_b32, whatever its spelling)
#define DESCENT_KEY(load, w, p) ((u64)(0xFFFFu - wave_bytes_code(load)) << 48 | (u64)(0xFFFFu - wave_bytes_code(w)) << 32 | (u64)(uint32_t)(p))

// L(b*) + w + min_gain < L(a) without overflow: the loads and w stay below 2^62, min_gain is any u64
__device__ __forceinline__ bool descent_gains(u64 la, u64 best, u64 w, u64 min_gain) { return !(la <= best + w || la - best - w <= min_gain); }

// a bid: atomicMin only lowers a word, so a word already at or below the key needs no atomic (all the proposals of one source collide
// there; most of them find a lower key in place).  Scope: __HIP_MEMORY_SCOPE_AGENT for a word in HBM, _WORKGROUP for one in LDS.
template <int Scope>
__device__ __forceinline__ void descent_bid(u64 *word, u64 key) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, Scope) > key) atomicMin(word, key);
}

// ---- the all-pairs rank of the descents over all brokers: how many brokers x are AHEAD of b, all pairs tiled through LDS.  By load:
// load[x] > mine, mine = load[b].  Cap, by utilisation: load[x] * mcap > mine * capacity[x], mcap = capacity[b]; loads and capacities
// stay below 2^62, so the products fit 128 bits.  Ties: x < b.  Every lane of a workgroup of T calls it (two barriers per tile); a
// lane with b >= B passes mine = 0, mcap = 1 and drops the result.  Static LDS: 8 T bytes, 16 T with Cap.  First (by load only):
// the brokers with first[x] != 0 rank before all others; bit 63 of a tile entry carries the flag (the loads stay below 2^62), and
// `mine` comes with it set for such a b.
template <int T, bool Cap, bool First = false>
__device__ __forceinline__ int rank_ahead(int B, int b, u64 mine, u64 mcap, const u64 *__restrict__ load, const u64 *__restrict__ capacity,
                                          const uint8_t *__restrict__ first = nullptr) {
    static_assert(!(Cap && First), "a first group is ranked by load only");
    __shared__ u64 tile[T], tcap[Cap ? T : 1];   // (tcap is never touched without Cap, and takes no LDS then)
    int r = 0;
    for (int base = 0; base < B; base += T) {
        const int cnt = min(T, B - base);
        if ((int)threadIdx.x < cnt) {
            tile[threadIdx.x] = load[base + threadIdx.x] | (First && first[base + threadIdx.x] ? 1ull << 63 : 0);
            if (Cap) tcap[threadIdx.x] = capacity[base + threadIdx.x];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            if constexpr (Cap) {
                const u128 theirs = (u128)tile[j] * mcap, ours = (u128)mine * tcap[j];
                r += (theirs > ours || (theirs == ours && base + j < b)) ? 1 : 0;
            } else {
                const u64 x = tile[j];
                r += (x > mine || (x == mine && base + j < b)) ? 1 : 0;
            }
        }
        __syncthreads();
    }
    return r;
}

}  // namespace
