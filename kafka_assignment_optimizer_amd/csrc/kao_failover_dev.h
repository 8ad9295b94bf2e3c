// kao_failover_dev.h -- what kao_failover_order (kao_failover.hip) and kao_failover_order_weighted
// (kao_wfailover.hip, section 4l) share: the scenario model's passes over the partitions (classify and scatter; the offsets between
// them are k_bucket_offsets of kao_plan_dev.h), the host function that runs them (fo_prelude) and the host-side checks of the
// arguments.  Included by those two .hip files only: everything sits in an unnamed namespace, so each gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kao_host.h"
#include "kao_plan_dev.h"   // k_bucket_offsets

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

__global__ void k_fo_scatter(int P, const int32_t *__restrict__ scen_of, const uint16_t *__restrict__ meta, const int32_t *__restrict__ start,
                             int32_t *__restrict__ fill, int32_t *__restrict__ list) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P || (meta[p] & 0xFF) == 0) return;
    const int g = scen_of[p];
    list[start[g] + atomicAdd(&fill[g], 1)] = p;
}

// The scenarios of one call on the device: classify, offsets and scatter enqueued on `st` and awaited.  *max_n = the affected
// partitions of the largest scenario, *threads = the lanes of a scenario's workgroup for it.  `solve` is the caller's scenario kernel,
// opened here for `lds` bytes of dynamic LDS when that is more than `lds_free` (what a launch may ask for unopened) and more than it
// has been opened for on this device.
struct FoScen {
    int32_t *lead, *scen_of, *cnt, *off, *start, *fill, *list, *claim, *ctl;   // [B], [P], [G] x 4, [P], [P], [FS_N]
    uint16_t *meta;                                                            // [P]
    uint8_t *cur;                                                              // [P]
};
int fo_prelude(hipStream_t st, int P, int W, int G, int scope, const uint16_t *d_rows, const uint8_t *d_rack, const FoScen &d, const void *solve,
               size_t lds, size_t lds_free, int *launches, int *max_n, int *threads) {
    const unsigned pblocks = grid_for(P, kFoThreads);
    if (P) {
        k_fo_classify<<<pblocks, kFoThreads, 0, st>>>(P, W, scope, d_rows, d_rack, d.lead, d.scen_of, d.meta, d.cur, d.claim, d.cnt, d.off);
        ++*launches;
    }
    k_bucket_offsets<<<1, 1024, 0, st>>>(G, d.cnt, nullptr, d.start, d.fill, d.ctl + FS_MAXN);   // start[], fill[] = 0, ctl[FS_MAXN] = the largest cnt
    ++*launches;
    if (P) {
        k_fo_scatter<<<pblocks, kFoThreads, 0, st>>>(P, d.scen_of, d.meta, d.start, d.fill, d.list);
        ++*launches;
    }
    HIP_TRY(hipGetLastError());
    int32_t ctl[FS_N];
    HIP_TRY(hipMemcpyAsync(ctl, d.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *max_n = ctl[FS_MAXN];
    *threads = (int64_t)*max_n * W <= kFoSmallSlots ? kFoSoloSmall : kFoSoloLarge;
    static int lds_set[kMaxDevices] = {0};   // the largest dynamic LDS size the kernel has been opened for, per device
    const int dev = cur_device();
    if (lds > lds_free && dev >= 0 && dev < kMaxDevices && (int)lds > lds_set[dev]) {
        HIP_TRY(hipFuncSetAttribute(solve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        lds_set[dev] = (int)lds;
    }
    return KAO_OK;
}

int validate_failover(const std::string &fn, int32_t B, int32_t R, const uint8_t *rack_of, int32_t P, int32_t W, const uint16_t *rows, int32_t scope,
                      const void *scen, const int32_t *n_reordered) {
    if (!rack_of || !rows || !scen || !n_reordered) return fail(KAO_ERR_INVALID, fn + "null pointer");
    if (scope < 0 || scope > 1) return fail(KAO_ERR_INVALID, fn + "scope must be 0 (brokers) or 1 (racks)");
    int rc = check_dims(fn, B, P, W, R);
    if (!rc) rc = check_slot_cap(fn, P, W);
    if (rc) return rc;
    if (B > kFoMaxBrokers) return fail(KAO_ERR_UNSUPPORTED, fn + "more than " + std::to_string(kFoMaxBrokers) + " brokers (the node state of a scenario lives in LDS)");
    for (int b = 0; b < B; ++b)
        if (rack_of[b] >= R) return fail(KAO_ERR_INVALID, fn + "rack_of[" + std::to_string(b) + "] >= n_racks");
    return check_rows(fn, B, P, W, rows);
}

}  // namespace
