// kao_failover_dev.h -- what kao_failover_order (kao_failover.hip) and kao_failover_order_weighted
// (kao_wfailover.hip, section 4l) share: the scenario model's passes over the partitions (classify, offsets, scatter), the host-side
// checks of the arguments and the holder of one call's device memory.  Included by those two .hip files only: everything sits in an
// unnamed namespace, so each gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kao_host.h"

namespace {

constexpr int kFoThreads = 256;         // the passes over partitions
constexpr int kFoSoloSmall = 256;       // lanes of a scenario's workgroup while the largest scenario has at most kFoSmallSlots slots
constexpr int kFoSoloLarge = 1024;
constexpr int kFoSmallSlots = 1024;
constexpr int kFoMaxBrokers = KAO_FAILOVER_MAX_BROKERS;   // 16 bytes of LDS per broker + the bitmap: 129,000 of 163,840 bytes
enum { FS_SCEN = 0, FS_PROBES = 1, FS_PHASES = 2, FS_ROUNDS = 3, FS_PATHS = 4, FS_MAXLEN = 5, FS_REORDERED = 6, FS_ERR = 7, FS_MAXN = 8, FS_N = 16 };

__device__ __forceinline__ bool fo_dead(int b, int g, int scope, const uint8_t *__restrict__ rack_of) {
    return scope == 0 ? b == g : rack_of[b] == g;
}

// meta[p] = e(p) | eligible slots << 8 (e = 0: offline); scen_of[p]; lead[]; the scenarios' affected / offline counts
__global__ void k_fo_classify(int P, int W, int scope, const uint16_t *__restrict__ rows, const uint8_t *__restrict__ rack_of,
                              int32_t *__restrict__ lead, int32_t *__restrict__ scen_of, uint16_t *__restrict__ meta,
                              uint8_t *__restrict__ cur, int32_t *__restrict__ claim, int32_t *__restrict__ cnt, int32_t *__restrict__ off) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const uint16_t *row = rows + (size_t)p * W;
    const int l = row[0], g = scope == 0 ? l : rack_of[l];
    int mask = 0, e = 0;
    for (int j = W - 1; j >= 1; --j) {
        const int b = row[j];
        if (b != KAO_NONE && !fo_dead(b, g, scope, rack_of)) { mask |= 1 << j; e = j; }
    }
    atomicAdd(&lead[l], 1);
    scen_of[p] = g;
    meta[p] = (uint16_t)(e | (mask << 8));
    cur[p] = (uint8_t)e;
    claim[p] = 0;
    atomicAdd(e ? &cnt[g] : &off[g], 1);
}

// start[g] = sum of cnt[0..g), fill[g] = 0; ctl[FS_MAXN] = the largest cnt.  One workgroup.
__global__ __launch_bounds__(1024) void k_fo_offsets(int G, const int32_t *__restrict__ cnt, int32_t *__restrict__ start,
                                                      int32_t *__restrict__ fill, int32_t *__restrict__ ctl) {
    __shared__ int32_t part[1024];
    __shared__ int32_t mx;
    const int tid = threadIdx.x, NT = blockDim.x, per = (G + NT - 1) / NT, lo = min(tid * per, G), hi = min(lo + per, G);
    if (tid == 0) mx = 0;
    __syncthreads();
    int s = 0, m = 0;
    for (int g = lo; g < hi; ++g) { s += cnt[g]; m = max(m, cnt[g]); }
    part[tid] = s;
    if (m) atomicMax(&mx, m);
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < NT; ++i) { const int v = part[i]; part[i] = acc; acc += v; }
        ctl[FS_MAXN] = mx;
    }
    __syncthreads();
    s = part[tid];
    for (int g = lo; g < hi; ++g) { start[g] = s; fill[g] = 0; s += cnt[g]; }
}

__global__ void k_fo_scatter(int P, const int32_t *__restrict__ scen_of, const uint16_t *__restrict__ meta, const int32_t *__restrict__ start,
                             int32_t *__restrict__ fill, int32_t *__restrict__ list) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || (meta[p] & 0xFF) == 0) return;
    const int g = scen_of[p];
    list[start[g] + atomicAdd(&fill[g], 1)] = p;
}

// the device memory and the stream of one call, handed back to the runtime's pools on every return path
struct FoBufs {
    void *arena = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    ~FoBufs() {
        if (stream) { (void)hipStreamSynchronize(stream); stream_put(stream, cur_device()); }
        if (arena) arena_put(arena, cap, cur_device());
    }
};


int validate_failover(const std::string &fn, int32_t B, int32_t R, const uint8_t *rack_of, int32_t P, int32_t W, const uint16_t *rows, int32_t scope,
                      const void *scen, const int32_t *n_reordered) {
    if (!rack_of || !rows || !scen || !n_reordered) return fail(KAO_ERR_INVALID, fn + "null pointer");
    if (scope < 0 || scope > 1) return fail(KAO_ERR_INVALID, fn + "scope must be 0 (brokers) or 1 (racks)");
    if (W < 1 || W > KAO_MAX_RF) return fail(KAO_ERR_INVALID, fn + "width outside 1.." + std::to_string(KAO_MAX_RF));
    if (B < 1 || B > 65534) return fail(KAO_ERR_INVALID, fn + "n_brokers outside 1..65534");
    if (R < 1 || R > KAO_MAX_RACKS) return fail(KAO_ERR_INVALID, fn + "n_racks outside 1.." + std::to_string(KAO_MAX_RACKS));
    if (P < 0) return fail(KAO_ERR_INVALID, fn + "n_partitions < 0");
    if ((int64_t)P * W > 4000000) return fail(KAO_ERR_UNSUPPORTED, fn + "more than 4,000,000 replica slots");
    if (B > kFoMaxBrokers) return fail(KAO_ERR_UNSUPPORTED, fn + "more than " + std::to_string(kFoMaxBrokers) + " brokers (the node state of a scenario lives in LDS)");
    for (int b = 0; b < B; ++b)
        if (rack_of[b] >= R) return fail(KAO_ERR_INVALID, fn + "rack_of[" + std::to_string(b) + "] >= n_racks");
    for (int64_t p = 0; p < P; ++p) {
        const uint16_t *row = rows + p * W;
        const std::string at = fn + "partition " + std::to_string(p) + ": ";
        if (row[0] == KAO_NONE) return fail(KAO_ERR_INVALID, at + "slot 0 holds no broker");
        bool ended = false;
        for (int i = 0; i < W; ++i) {
            if (row[i] == KAO_NONE) { ended = true; continue; }
            if (ended) return fail(KAO_ERR_INVALID, at + "a broker after an empty slot");
            if (row[i] >= B) return fail(KAO_ERR_INVALID, at + "broker index >= n_brokers");
            for (int j = 0; j < i; ++j)
                if (row[j] == row[i]) return fail(KAO_ERR_INVALID, at + "broker repeated in a row");
        }
    }
    return KAO_OK;
}

}  // namespace
