// kao_waves.hip -- kao_plan_waves: a reassignment plan split into waves with at most k partition movements per broker per wave;
// kao_plan_waves_sized: the same with a cap on the bytes each broker moves per wave;
// kao_plan_waves_headroom: waves as a sequence of states in which no broker holds more than its capacity (section 4v, further
// down).  Kernels and the C entry points.
//
// A partition p that changed and adds brokers (add(p) = target \ current) moves data: its participants S(p) are add(p) plus the
// copy source current[p][0] (new followers fetch from the leader).  The waves are a first fit: partitions in a priority order,
// each into the first wave where every participant has fewer than k movements.  The GPU runs that sequential first fit EXACTLY,
// for kWaveOrders priority orders at once, in rounds:
//   - minkey[o][b] = lowest key among the still unplaced partitions of order o at broker b (one 64-bit atomicMin per participant);
//   - an unplaced p whose key is minkey[o][b] at EVERY participant b has no unplaced partition ahead of it at any of its brokers,
//     so the loads it sees are exactly the ones the sequential first fit would see: it is placed now.  Two partitions placed in
//     one round share no broker (each broker has one minimum), so the load updates need no atomics;
//   - every other unplaced p bids into the next round's minkey.
// The round's lowest key is always placed, so the rounds end; a broker places at most one partition per round, so the round
// count is at least the largest participant degree.  Keys are unique within an order ((~maxdeg) << 32 | a bijection of p), so
// the result depends on (input, seed) only.  Order 0 is degree-descending, ties by partition index; orders 1.. break the ties by
// a seeded bijective hash.  The order with the fewest waves wins (ties: the lowest order).
//
// Sized (kao_plan_waves_sized): participant b of p carries traffic t_p(b) = size[p] at an added broker, n_added(p) * size[p] at
// the source.  The fit test at b adds "load_bytes == 0 || load_bytes + t_p(b) <= C" (C = 0: no byte cap) to the count test
// (k = 0: no count cap); a partition above C thus goes alone.  The key's high word becomes (~code(max_b t_p(b))) << 16 |
// ~min(maxdeg, 0xFFFF), so order 0 is first fit decreasing by traffic.  The rounds are unchanged: the argument above holds for
// any fit test that depends on the loads a partition sees.
//
// Layout: the row walk (wave_each_added / wave_each_removed) that every kernel and host check of add(p) and rem(p) goes through;
// the kernels of the plain and sized calls; the kernels of the headroom call; the host checks; then the host flow.  All three
// calls share their front half (wave_front: buffers, uploads, k_wave_classify, k_wave_bound) and their tail (wave_tail: the one
// scatter kernel, wave[] read back, the lower bound); each keeps its own round loop between the two, since the loops end on
// different conditions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "kao_bytes_code.h"   // wave_bytes_code
#include "kao_host.h"

namespace {

constexpr int kWaveOrders = 64;              // priority orders per launch (each its own slice of loads / minkeys)
constexpr int kWavePart = KAO_MAX_RF + 1;    // participants per partition: up to KAO_MAX_RF added brokers + the source
constexpr int kWaveThreads = 256;
constexpr int kWaveBatch = 32;               // rounds enqueued between two checks of the "anything left" flag
constexpr size_t kWaveBudget = size_t(1) << 30;  // device bytes the per-order state may take; fewer orders when it would not fit
enum { CTL_NMV = 0, CTL_CHANGED = 1, CTL_LB = 2, CTL_WCAP = 3, CTL_ERR = 4, CTL_N = 8 };

// The row walk: f(broker) for every broker of row `of` that row `other` does not hold, in the slot order of `of`.
template <class F>
__host__ __device__ inline void wave_each_missing(const uint16_t *of, const uint16_t *other, int W, F f) {
    for (int i = 0; i < W; ++i) {
        const uint16_t b = of[i];
        if (b == KAO_NONE) continue;
        bool held = false;
        for (int j = 0; j < W; ++j) held |= other[j] == b;
        if (!held) f(b);
    }
}

// add(p) = target \ current in target-slot order: the order fixes the participant order and the source's place in part[]
template <class F>
__host__ __device__ inline void wave_each_added(const uint16_t *cur, const uint16_t *tgt, int W, F f) { wave_each_missing(tgt, cur, W, f); }

// rem(p) = current \ target in current-slot order
template <class F>
__host__ __device__ inline void wave_each_removed(const uint16_t *cur, const uint16_t *tgt, int W, F f) { wave_each_missing(cur, tgt, W, f); }

__host__ __device__ inline uint32_t wave_mix32(uint32_t x) {  // murmur3 finaliser: a bijection of 32-bit words
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

__host__ __device__ inline uint32_t wave_salt(uint64_t seed, uint32_t o) {  // splitmix64 of (seed, order), low word
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(o + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}

// priority key of partition p in order o: smaller = earlier.  Unique within an order for p < 2^32.  khi is the partition's high
// word (k_wave_bound): ~maxdeg for the count-only planner, ~traffic code and ~degree for the sized one.
__device__ inline uint64_t wave_key(uint32_t o, uint32_t p, uint32_t khi, uint32_t salt) {
    const uint32_t tie = o == 0 ? p : wave_mix32(p ^ salt);
    return (uint64_t)khi << 32 | tie;
}

// wavefront-aggregated atomics on the few global control words (one atomic per wavefront, all 64 lanes must be active)
__device__ inline int wave_reserve(bool take, int32_t *counter) {
    const unsigned long long m = __ballot(take);
    if (m == 0ull) return -1;
    const int lane = __lane_id(), leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(m));
    base = __shfl(base, leader);
    return take ? base + __popcll(m & ((1ull << lane) - 1ull)) : -1;
}

__device__ inline void wave_max_to(int32_t v, int32_t *dst) {
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    if (__lane_id() == 0 && v > 0) atomicMax(dst, v);
}

// One thread per partition: unchanged -> wave -1; changed without an added broker -> wave 0 (moves no data); otherwise the
// partition joins the list of moving ones (slot order depends on timing; everything downstream is keyed by p, not by slot).
// Sized: also each participant's traffic traf[slot][j], and per broker tot[b] = T_b = sum of t_p(b) and clamp[b] = sum of
// min(t_p(b), C) (C = 0: no byte cap, clamp unused).
template <bool Sized>
__global__ void k_wave_classify(int32_t P, int32_t W, const uint16_t *__restrict__ cur, const uint16_t *__restrict__ tgt,
                                int32_t *__restrict__ wave, uint16_t *__restrict__ part, uint8_t *__restrict__ npart,
                                int32_t *__restrict__ mv_idx, int32_t *__restrict__ deg, int32_t *__restrict__ ctl,
                                const uint64_t *__restrict__ size, uint64_t C, uint64_t *__restrict__ traf,
                                unsigned long long *__restrict__ tot, unsigned long long *__restrict__ clamp) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint16_t c[KAO_MAX_RF], n[KAO_MAX_RF], s[kWavePart];
    bool changed = false;
    int ns = 0;
    if (p < P) {
        for (int i = 0; i < W; ++i) {
            c[i] = cur[p * W + i];
            n[i] = tgt[p * W + i];
            changed |= c[i] != n[i];
        }
        if (changed) {
            wave_each_added(c, n, W, [&](uint16_t b) { s[ns++] = b; });
            if (ns > 0 && c[0] != KAO_NONE) s[ns++] = c[0];
        }
        if (!changed) wave[p] = -1;
        else if (ns == 0) wave[p] = 0;
    }
    const int slot = wave_reserve(ns > 0, &ctl[CTL_NMV]);
    wave_max_to(changed ? 1 : 0, &ctl[CTL_CHANGED]);
    if (slot < 0) return;
    mv_idx[slot] = (int32_t)p;
    npart[slot] = (uint8_t)ns;
    for (int j = 0; j < ns; ++j) {
        part[(size_t)slot * kWavePart + j] = s[j];
        atomicAdd(&deg[s[j]], 1);
    }
    if constexpr (Sized) {
        const int n_added = c[0] != KAO_NONE ? ns - 1 : ns;   // the source, when there is one, is the last participant
        const uint64_t sz = size[p];
        for (int j = 0; j < ns; ++j) {
            const uint64_t t = j < n_added ? sz : (uint64_t)n_added * sz;   // no overflow: the host checked T_b < 2^62
            traf[(size_t)slot * kWavePart + j] = t;
            atomicAdd(&tot[s[j]], (unsigned long long)t);
            if (C) atomicAdd(&clamp[s[j]], (unsigned long long)(t < C ? t : C));
        }
    }
}

// One thread per moving partition: the high word of its key (khi), the lower bound and the wave cap.
// Count-only: khi = ~maxdeg, LB = max_b ceil(deg(b) / k), and p's first fit is at most sum_b floor((deg(b) - 1) / k) waves
// later than wave 0, since every wave before it is full at some participant.
// Sized: a wave before p's is blocked at some participant b, by count (at most floor((deg(b) - 1) / k) such waves, k >= 1) or
// by bytes (C >= 1: load > C - t_p(b) and load > 0; the other partitions at b carry T_b - t_p(b) bytes and give at most
// deg(b) - 1 nonzero loads, so at most min(deg(b) - 1, floor((T_b - t_p(b)) / max(1, C - t_p(b) + 1))) such waves).  wcap = 1 +
// max_p of the sum of both terms over p's participants.  LB = max_b of ceil(deg(b) / k) and ceil(clamp[b] / C), at least 1.
template <bool Sized>
__global__ void k_wave_bound(int32_t n_mv, int32_t k, const uint16_t *__restrict__ part, const uint8_t *__restrict__ npart,
                             const int32_t *__restrict__ deg, uint32_t *__restrict__ khi, int32_t *__restrict__ ctl, uint64_t C,
                             const uint64_t *__restrict__ traf, const unsigned long long *__restrict__ tot,
                             const unsigned long long *__restrict__ clamp) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t md = 0, cap = 0, lb = 0;
    if (i < n_mv) {
        uint64_t mt = 0;
        for (int j = 0; j < npart[i]; ++j) {
            const int b = part[(size_t)i * kWavePart + j];
            const int32_t d = deg[b];
            md = max(md, d);
            if constexpr (Sized) {
                if (k) cap += (d - 1) / k;
                const uint64_t t = traf[(size_t)i * kWavePart + j];
                mt = max(mt, t);
                if (C) {
                    const uint64_t rest = tot[b] - t;                  // bytes of the other partitions at b
                    uint64_t by = 0;
                    if (t > C) by = rest;                              // every nonzero load blocks p
                    else if (C - t < rest) by = rest / (C - t + 1);    // C - t + 1 <= rest: no overflow
                    cap += (int32_t)min<uint64_t>(by, (uint64_t)(d - 1));
                    const unsigned long long cl = clamp[b];
                    lb = max(lb, (int32_t)(cl / C + (cl % C != 0)));
                }
            } else {
                cap += (d - 1) / k;
            }
        }
        if constexpr (Sized) {
            khi[i] = (0xFFFFu - wave_bytes_code(mt)) << 16 | (0xFFFFu - (uint32_t)min(md, 0xFFFF));
            lb = max(lb, 1);   // a moving partition needs a wave even when every byte count is 0
        }
        else
            khi[i] = 0xFFFFFFFFu - (uint32_t)md;
        cap += 1;
        if (k) lb = max(lb, (md + k - 1) / k);
    }
    wave_max_to(lb, &ctl[CTL_LB]);
    wave_max_to(cap, &ctl[CTL_WCAP]);
}

// Round -1: every moving partition bids into the first round's minkeys.  grid = (slots, orders).
__global__ void k_wave_seed(int32_t n_mv, int32_t B, uint64_t seed, const uint16_t *__restrict__ part, const uint8_t *__restrict__ npart,
                            const int32_t *__restrict__ mv_idx, const uint32_t *__restrict__ khi, unsigned long long *__restrict__ mk0) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t o = blockIdx.y;
    if (i >= n_mv) return;
    const unsigned long long key = wave_key(o, (uint32_t)mv_idx[i], khi[i], wave_salt(seed, o));
    unsigned long long *mk = mk0 + (size_t)o * B;
    for (int j = 0; j < npart[i]; ++j) atomicMin(&mk[part[(size_t)i * kWavePart + j]], key);
}

// Round r: reads minkey buffer r % 3, bids into (r + 1) % 3, clears (r + 2) % 3 (read by round r - 1, written by round r + 1).
// flags[(r + 1) % 3] = 1 when a partition is still unplaced after this round.  loads[o][b][w] (movements; sized: only when k >= 1),
// bytes[o][b][w] (sized), waveo[o][slot] (-1 = unplaced).
template <bool Sized>
__global__ void k_wave_round(int32_t r, int32_t n_ord, int32_t n_mv, int32_t B, int32_t wcap, int32_t k, uint64_t seed,
                             const uint16_t *__restrict__ part, const uint8_t *__restrict__ npart, const int32_t *__restrict__ mv_idx,
                             const uint32_t *__restrict__ khi, unsigned long long *__restrict__ mk, int32_t *__restrict__ loads,
                             int32_t *__restrict__ waveo, int32_t *__restrict__ nw, int32_t *__restrict__ flags, int32_t *__restrict__ ctl,
                             uint64_t C, const uint64_t *__restrict__ traf, uint64_t *__restrict__ bytes) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t o = blockIdx.y;
    const size_t per = (size_t)n_ord * B;
    {   // clear the buffer of round r + 2
        const size_t nthreads = (size_t)gridDim.x * blockDim.x * gridDim.y;
        const size_t tid = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
        unsigned long long *clr = mk + (size_t)((r + 2) % 3) * per;
        for (size_t e = tid; e < per; e += nthreads) clr[e] = ~0ull;
        if (tid == 0) flags[(r + 2) % 3] = 0;
    }
    bool pending = false;
    if (i < n_mv && waveo[(size_t)o * n_mv + i] < 0) {
        const uint32_t p = (uint32_t)mv_idx[i];
        const unsigned long long key = wave_key(o, p, khi[i], wave_salt(seed, o));
        const int np = npart[i];
        uint16_t b[kWavePart];
        for (int j = 0; j < np; ++j) b[j] = part[(size_t)i * kWavePart + j];
        const unsigned long long *mine = mk + (size_t)(r % 3) * per + (size_t)o * B;
        bool ready = true;
        for (int j = 0; j < np; ++j) ready &= mine[b[j]] == key;
        if (ready) {
            int32_t *L = loads + (size_t)o * B * wcap;
            int32_t w = 0;
            if constexpr (Sized) {
                uint64_t t[kWavePart];
                for (int j = 0; j < np; ++j) t[j] = traf[(size_t)i * kWavePart + j];
                uint64_t *Y = bytes + (size_t)o * B * wcap;
                for (; w < wcap; ++w) {
                    bool fit = true;
                    for (int j = 0; j < np; ++j) {
                        const size_t e = (size_t)b[j] * wcap + w;
                        if (k) fit &= L[e] < k;
                        if (C) fit &= Y[e] == 0 || Y[e] + t[j] <= C;   // loads stay below 2^63: no overflow
                    }
                    if (fit) break;
                }
                if (w < wcap) {
                    for (int j = 0; j < np; ++j) {
                        const size_t e = (size_t)b[j] * wcap + w;
                        if (k) L[e] += 1;
                        Y[e] += t[j];
                    }
                }
            } else {
                for (; w < wcap; ++w) {
                    bool fit = true;
                    for (int j = 0; j < np; ++j) fit &= L[(size_t)b[j] * wcap + w] < k;
                    if (fit) break;
                }
                if (w < wcap)
                    for (int j = 0; j < np; ++j) L[(size_t)b[j] * wcap + w] += 1;
            }
            if (w < wcap) {
                waveo[(size_t)o * n_mv + i] = w;
                atomicMax(&nw[o], w + 1);
            } else {
                atomicOr(&ctl[CTL_ERR], 1);  // cannot happen (wcap bounds every first fit); the host stops on it
            }
        } else {
            unsigned long long *next = mk + (size_t)((r + 1) % 3) * per + (size_t)o * B;
            for (int j = 0; j < np; ++j) atomicMin(&next[b[j]], key);
            pending = true;
        }
    }
    wave_max_to(pending ? 1 : 0, &flags[(r + 1) % 3]);
}

// The winning order's waves by partition, for all three calls: -2 for a slot left without a wave (stuck, headroom only: the other
// two calls place every slot or fail).
__global__ void k_wave_scatter(int32_t n_mv, const int32_t *__restrict__ waveo, const int32_t *__restrict__ mv_idx, int32_t *__restrict__ wave) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_mv) wave[mv_idx[i]] = waveo[i] < 0 ? -2 : waveo[i];
}

// ---- kao_plan_waves_headroom: waves as a sequence of states, each of which fits every disk ----
//
// Per order o, in global memory: occ / arr / dep / byt (u64) and cnt (i32) over the brokers, three rotating minkey rows, waveo[slot]
// (-1 = undecided or stuck), skipw[slot] = the wave in which the slot last decided "skip" (so nothing is reset between waves), and
// the words of HeadOrder.  An order works on ONE wave at a time (its loads are the open wave's), and orders sit at different waves
// within one launch.
//
// k_head_round, round r: an undecided slot that did not skip the open wave tests the fit (the sized test at its participants, the
// headroom test occ + arr + size <= capacity at add(p)) against the loads as they stand.  Every test only turns from true to false
// within a wave, and the only stores to the loads a slot reads come from slots with a lower key at that broker (the holder of a
// broker's minimum), which the sequential pass visits earlier: failing now is failing there, so the slot skips the wave at once,
// without bidding.  A slot that fits and holds the minimum of the previous round's bids at every participant has no undecided
// fitting slot ahead of it at any of its brokers: the loads it just tested are the sequential ones, and it joins with plain
// stores (two joiners of one round share no participant).  dep[] at rem(p) is read by the close step only, so it takes an
// atomicAdd there and rem(p) is not bid at: shorter chains, and 9 rather than 17 brokers per slot.  Every other fitting slot
// bids its key into the next round's row.
//
// k_head_close, after every round, one workgroup per order: when the round had no bidder the open wave is complete.  It records
// the least free bytes over the brokers with arr > 0, does occ += arr - dep, clears the wave's loads, advances the wave, and
// marks the order done when the wave was idle (no joiner, dep 0 everywhere).  Fusing the close into the round would need a
// barrier over the order's workgroups between a round's last store and the next round's first test; a launch boundary is that
// barrier, and a closing workgroup that has nothing to do exits after two loads.
struct HeadOrder {
    int32_t wave;      // the open wave
    int32_t took;      // a slot joined the open wave
    int32_t done;      // the first idle wave was seen
    int32_t n_waves;   // 1 + the last wave that holds a moving partition
    int32_t bid[3];    // bid[(r + 1) % 3] != 0: round r had a bidder
    int32_t mf_wave, mf_broker;
    int32_t stuck;
    unsigned long long mf;   // least free bytes so far, ~0 = none
};

__device__ inline uint64_t ld64(const uint64_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ inline void st64(uint64_t *p, uint64_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
__device__ inline int32_t ld32(const int32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ inline void st32(int32_t *p, int32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }

// One thread per partition: dep0[b] = bytes that leave b in wave 0 with the metadata-only partitions (changed, nothing added).
__global__ void k_head_dep0(int32_t P, int32_t W, const uint16_t *__restrict__ cur, const uint16_t *__restrict__ tgt,
                            const uint64_t *__restrict__ size, unsigned long long *__restrict__ dep0) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    uint16_t c[KAO_MAX_RF], n[KAO_MAX_RF];
    bool changed = false;
    for (int i = 0; i < W; ++i) {
        c[i] = cur[p * W + i];
        n[i] = tgt[p * W + i];
        changed |= c[i] != n[i];
    }
    if (!changed || size[p] == 0) return;
    bool adds = false;
    wave_each_added(c, n, W, [&](uint16_t) { adds = true; });
    if (adds) return;   // any added broker: the partition moves data and leaves with its own wave
    wave_each_removed(c, n, W, [&](uint16_t b) { atomicAdd(&dep0[b], (unsigned long long)size[p]); });
}

// grid = (brokers / 256, orders): every order starts from occ = stored and wave 0's departures.
__global__ void k_head_init(int32_t B, const uint64_t *__restrict__ stored, const unsigned long long *__restrict__ dep0,
                            uint64_t *__restrict__ occ, uint64_t *__restrict__ dep) {
    const int32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const size_t e = (size_t)blockIdx.y * B + b;
    occ[e] = stored[b];
    dep[e] = dep0[b];
}

__global__ void k_head_round(int32_t r, int32_t n_ord, int32_t n_mv, int32_t B, int32_t W, int32_t k, uint64_t C, uint64_t seed,
                             const uint16_t *__restrict__ cur, const uint16_t *__restrict__ tgt, const uint64_t *__restrict__ size,
                             const uint64_t *__restrict__ capacity, const uint16_t *__restrict__ part,
                             const uint8_t *__restrict__ npart, const int32_t *__restrict__ mv_idx, const uint32_t *__restrict__ khi,
                             const uint64_t *__restrict__ traf, unsigned long long *__restrict__ mk, uint64_t *__restrict__ occ,
                             uint64_t *__restrict__ arr, uint64_t *__restrict__ dep, uint64_t *__restrict__ byt, int32_t *__restrict__ cnt,
                             int32_t *__restrict__ waveo, int32_t *__restrict__ skipw, HeadOrder *__restrict__ ord) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t o = blockIdx.y;
    HeadOrder *ho = ord + o;
    if (ho->done) return;   // uniform over the order's workgroups: written by the close step only
    const size_t per = (size_t)n_ord * B, ob = (size_t)o * B;
    {   // clear this order's row of round r + 2 (read by round r - 1, bid into by round r + 1)
        unsigned long long *clr = mk + (size_t)((r + 2) % 3) * per + ob;
        for (int32_t e = i; e < B; e += gridDim.x * blockDim.x) clr[e] = ~0ull;
        if (i == 0) ho->bid[(r + 2) % 3] = 0;
    }
    const int32_t w = ho->wave;
    bool bids = false;
    const size_t os = (size_t)o * n_mv + (i < n_mv ? i : 0);
    if (i < n_mv && waveo[os] < 0 && skipw[os] != w) {
        const int32_t p = mv_idx[i];
        const int np = npart[i];
        const int n_added = cur[(size_t)p * W] != KAO_NONE ? np - 1 : np;   // the source, when there is one, is the last participant
        const uint64_t sz = size[p];
        const uint16_t *pb = part + (size_t)i * kWavePart;   // re-read per loop rather than kept in a runtime-indexed array
        const uint64_t *pt = traf + (size_t)i * kWavePart;
        bool fit = true;
        for (int j = 0; j < np; ++j) {
            const size_t e = ob + pb[j];
            if (k) fit &= ld32(&cnt[e]) < k;
            if (C) {
                const uint64_t l = ld64(&byt[e]);
                fit &= l == 0 || l + pt[j] <= C;                        // loads stay below 2^63: no overflow
            }
            if (j < n_added && sz)                                      // occ + arr < 2^63, size < 2^62: no overflow
                fit &= ld64(&occ[e]) + ld64(&arr[e]) + sz <= capacity[pb[j]];
        }
        if (!fit) {
            skipw[os] = w;
        } else {
            const unsigned long long key = wave_key(o, (uint32_t)p, khi[i], wave_salt(seed, o));
            const unsigned long long *mine = mk + (size_t)(r % 3) * per + ob;
            bool ready = true;
            for (int j = 0; j < np; ++j) ready &= mine[pb[j]] == key;
            if (ready) {
                for (int j = 0; j < np; ++j) {
                    const size_t e = ob + pb[j];
                    if (k) st32(&cnt[e], cnt[e] + 1);
                    if (C) st64(&byt[e], byt[e] + pt[j]);
                    if (j < n_added) st64(&arr[e], arr[e] + sz);
                }
                if (sz) {
                    // rem(p) = current \ target, written out: through wave_each_removed the compiler emits other code for this kernel
                    for (int c = 0; c < W; ++c) {
                        const uint16_t cb = cur[(size_t)p * W + c];
                        if (cb == KAO_NONE) continue;
                        bool kept = false;
                        for (int j = 0; j < W; ++j) kept |= tgt[(size_t)p * W + j] == cb;
                        if (!kept) atomicAdd(reinterpret_cast<unsigned long long *>(&dep[ob + cb]), (unsigned long long)sz);
                    }
                }
                waveo[os] = w;
                st32(&ho->took, 1);
            } else {
                unsigned long long *next = mk + (size_t)((r + 1) % 3) * per + ob;
                for (int j = 0; j < np; ++j) atomicMin(&next[pb[j]], key);
                bids = true;
            }
        }
    }
    if (__ballot(bids) != 0ull && __lane_id() == 0) st32(&ho->bid[(r + 1) % 3], 1);
}

// grid = orders, one workgroup each, after round r.  n_done counts the orders that have seen their idle wave.
__global__ void __launch_bounds__(kWaveThreads) k_head_close(int32_t r, int32_t B, const uint64_t *__restrict__ capacity,
                                                             uint64_t *__restrict__ occ, uint64_t *__restrict__ arr, uint64_t *__restrict__ dep,
                                                             uint64_t *__restrict__ byt, int32_t *__restrict__ cnt, HeadOrder *__restrict__ ord,
                                                             int32_t *__restrict__ n_done) {
    __shared__ unsigned long long s_free[kWaveThreads];
    __shared__ int32_t s_b[kWaveThreads];
    __shared__ int32_t s_dep[kWaveThreads];
    HeadOrder *ho = ord + blockIdx.x;
    if (ho->done || ho->bid[(r + 1) % 3]) return;   // uniform over the workgroup
    const size_t ob = (size_t)blockIdx.x * B;
    unsigned long long mf = ~0ull;
    int32_t mb = -1, any_dep = 0;
    for (int32_t b = threadIdx.x; b < B; b += kWaveThreads) {   // ascending b per thread: the first minimum is the lowest broker
        const uint64_t a = arr[ob + b], d = dep[ob + b];
        any_dep |= d != 0;
        if (a) {
            // the fit test held: no wrap; clamped as it is reported, before every comparison (here, the reduction, ho->mf)
            const uint64_t fr = std::min<uint64_t>(capacity[b] - occ[ob + b] - a, (uint64_t)INT64_MAX);
            if (fr < mf) { mf = fr; mb = b; }
        }
        if (a | d) occ[ob + b] += a - d;                          // stored >= every departure (host check): no wrap
        arr[ob + b] = 0;
        dep[ob + b] = 0;
        byt[ob + b] = 0;
        cnt[ob + b] = 0;
    }
    s_free[threadIdx.x] = mf;
    s_b[threadIdx.x] = mb;
    s_dep[threadIdx.x] = any_dep;
    __syncthreads();
    for (int off = kWaveThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const unsigned long long f2 = s_free[threadIdx.x + off];
            const int32_t b2 = s_b[threadIdx.x + off];
            if (b2 >= 0 && (s_b[threadIdx.x] < 0 || f2 < s_free[threadIdx.x] || (f2 == s_free[threadIdx.x] && b2 < s_b[threadIdx.x]))) {
                s_free[threadIdx.x] = f2;
                s_b[threadIdx.x] = b2;
            }
            s_dep[threadIdx.x] |= s_dep[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int32_t w = ho->wave;
        if (s_b[0] >= 0 && (ho->mf_broker < 0 || s_free[0] < ho->mf)) {   // strictly less: the earliest wave keeps a tie
            ho->mf = s_free[0];
            ho->mf_wave = w;
            ho->mf_broker = s_b[0];
        }
        if (ho->took) ho->n_waves = w + 1;
        if (!ho->took && !s_dep[0]) {
            ho->done = 1;
            atomicAdd(n_done, 1);
        }
        ho->took = 0;
        ho->wave = w + 1;
    }
}

// grid = (slots / 256, orders): the stuck slots of every order.
__global__ void k_head_tally(int32_t n_mv, const int32_t *__restrict__ waveo, HeadOrder *__restrict__ ord) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = __ballot(i < n_mv && waveo[(size_t)blockIdx.y * n_mv + (i < n_mv ? i : 0)] < 0);
    if (m != 0ull && __lane_id() == 0) atomicAdd(&ord[blockIdx.y].stuck, __popcll(m));
}

// device buffers of one call, released on every return path (not CallBufs of kao_host.h: a call allocates up to 1 GiB, which must
// not be parked in the arena pool)
struct WaveBufs {
    std::vector<void *> ptrs;
    hipStream_t stream = nullptr;
    template <typename T>
    int alloc(T **p, size_t n) {
        *p = nullptr;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), std::max<size_t>(n, 1) * sizeof(T)));
        ptrs.push_back(*p);
        return KAO_OK;
    }
    ~WaveBufs() {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        for (void *p : ptrs) (void)hipFree(p);
    }
};

int validate_waves(const char *fn, int32_t B, int32_t P, int32_t W, const uint16_t *cur, const uint16_t *tgt, const int32_t *wave,
                   const int32_t *n_waves, const int32_t *lower_bound) {
    const std::string f = fn;
    if (!cur || !tgt || !wave || !n_waves || !lower_bound) return fail(KAO_ERR_INVALID, f + ": null pointer");
    if (W < 1 || W > KAO_MAX_RF) return fail(KAO_ERR_INVALID, f + ": width must be 1.." + std::to_string(KAO_MAX_RF));
    if (B < 1 || B > 65534) return fail(KAO_ERR_INVALID, f + ": n_brokers must be 1..65534");
    if (P < 0) return fail(KAO_ERR_INVALID, f + ": n_partitions < 0");
    for (int64_t p = 0; p < P; ++p) {
        for (int side = 0; side < 2; ++side) {
            const uint16_t *row = (side ? tgt : cur) + p * W;
            int filled = 0;
            for (int i = 0; i < W; ++i) {
                if (row[i] == KAO_NONE) continue;
                if (row[i] >= B)
                    return fail(KAO_ERR_INVALID, f + ": partition " + std::to_string(p) + ": broker index " + std::to_string(row[i]) + " >= n_brokers");
                for (int j = 0; j < i; ++j)
                    if (row[j] == row[i]) return fail(KAO_ERR_INVALID, f + ": partition " + std::to_string(p) + ": broker repeated in a row");
                ++filled;
            }
            if (side == 1 && filled == 0) return fail(KAO_ERR_INVALID, f + ": partition " + std::to_string(p) + ": target row has no broker");
        }
    }
    return KAO_OK;
}

// T_b, the bytes broker b moves over the whole plan, with overflow-checked arithmetic: every load and every load + t_p(b) of the
// kernel then stays below 2^63.  KAO_ERR_INVALID when some T_b reaches 2^62.  Rows are valid (validate_waves).
int validate_traffic(const char *fn, int32_t B, int32_t P, int32_t W, const uint16_t *cur, const uint16_t *tgt, const uint64_t *size) {
    constexpr uint64_t kLimit = uint64_t(1) << 62;
    std::vector<uint64_t> tot((size_t)B, 0);
    for (int64_t p = 0; p < P; ++p) {
        const uint16_t *c = cur + p * W, *n = tgt + p * W;
        uint16_t add[KAO_MAX_RF];
        int na = 0;
        wave_each_added(c, n, W, [&](uint16_t b) { add[na++] = b; });
        if (na == 0) continue;   // unchanged, or changed without moving data
        uint64_t src = 0;
        bool bad = __builtin_mul_overflow(size[p], (uint64_t)na, &src);
        for (int j = 0; j < na && !bad; ++j) bad = __builtin_add_overflow(tot[add[j]], size[p], &tot[add[j]]) || tot[add[j]] >= kLimit;
        if (!bad && c[0] != KAO_NONE) bad = __builtin_add_overflow(tot[c[0]], src, &tot[c[0]]) || tot[c[0]] >= kLimit;
        if (bad)
            return fail(KAO_ERR_INVALID, std::string(fn) + ": partition " + std::to_string(p) + ": a broker's traffic reaches 2^62 bytes");
    }
    return KAO_OK;
}

// stored[b] against the bytes that leave b over the whole plan (rem(p) = current \ target of every changed partition), and the
// 2^62 limit.  Rows are valid (validate_waves).
int validate_stored(const char *fn, int32_t B, int32_t P, int32_t W, const uint16_t *cur, const uint16_t *tgt, const uint64_t *size,
                    const uint64_t *stored) {
    constexpr uint64_t kLimit = uint64_t(1) << 62;
    const std::string f = fn;
    for (int32_t b = 0; b < B; ++b)
        if (stored[b] >= kLimit) return fail(KAO_ERR_INVALID, f + ": stored[" + std::to_string(b) + "] reaches 2^62 bytes");
    std::vector<uint64_t> left(stored, stored + B);
    for (int64_t p = 0; p < P; ++p) {
        const uint16_t *c = cur + p * W, *n = tgt + p * W;
        int short_of = -1;   // the first broker of rem(p) that holds less than leaves it
        wave_each_removed(c, n, W, [&](uint16_t b) {
            if (short_of >= 0) return;
            if (left[b] < size[p]) short_of = b;
            else left[b] -= size[p];
        });
        if (short_of >= 0)
            return fail(KAO_ERR_INVALID, f + ": stored[" + std::to_string(short_of) + "] is below the bytes of the partitions that leave the broker (partition " +
                                             std::to_string(p) + ")");
    }
    return KAO_OK;
}

// The number of priority orders whose state (per_order bytes each) fits the budget.
int wave_orders(size_t per_order) { return (int)std::max<size_t>(1, std::min<size_t>(kWaveOrders, kWaveBudget / per_order)); }

// What every call holds once its partitions are classified and bounded: the stream and the buffers (released with it), the
// device pointers the later kernels take, the grids, and the control words as k_wave_bound left them.
struct WaveFront {
    WaveBufs m;
    hipStream_t st = nullptr;
    uint16_t *cur, *tgt, *part;
    uint8_t *npart;
    int32_t *wave, *mv, *deg, *d_ctl;
    uint32_t *khi;
    uint64_t *size = nullptr, *traf = nullptr;               // sized calls only
    unsigned long long *tot = nullptr, *clamp = nullptr;     // sized calls only
    int32_t n_mv = 0;                                        // moving partitions (slots)
    unsigned pblocks = 0, mblocks = 0;                       // workgroups over the partitions / over the slots
    int32_t ctl[CTL_N];
};

// The front half of every call: buffers, uploads, k_wave_classify and, when a partition moves, k_wave_bound.  Sized: size != nullptr,
// C = max_bytes_per_broker (0 = no byte cap), k = 0 = no count cap.
template <bool Sized>
int wave_front(WaveFront &f, int32_t B, int32_t P, int32_t W, const uint16_t *current, const uint16_t *target, const uint64_t *size, uint64_t C,
               int32_t k) {
    WaveBufs &m = f.m;
    HIP_TRY(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking));
    const hipStream_t st = f.st = m.stream;
    int rc;
    const size_t PW = (size_t)P * W;
    if ((rc = m.alloc(&f.cur, PW)) || (rc = m.alloc(&f.tgt, PW)) || (rc = m.alloc(&f.part, (size_t)P * kWavePart)) ||
        (rc = m.alloc(&f.npart, (size_t)P)) || (rc = m.alloc(&f.wave, (size_t)P)) || (rc = m.alloc(&f.mv, (size_t)P)) ||
        (rc = m.alloc(&f.deg, (size_t)B)) || (rc = m.alloc(&f.khi, (size_t)P)) || (rc = m.alloc(&f.d_ctl, CTL_N)))
        return rc;
    if (Sized && ((rc = m.alloc(&f.size, (size_t)P)) || (rc = m.alloc(&f.traf, (size_t)P * kWavePart)) ||
                  (rc = m.alloc(&f.tot, (size_t)B)) || (rc = m.alloc(&f.clamp, (size_t)B))))
        return rc;
    HIP_TRY(hipMemcpyAsync(f.cur, current, PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(f.tgt, target, PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(f.deg, 0, (size_t)B * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(f.d_ctl, 0, CTL_N * sizeof(int32_t), st));
    if (Sized) {
        HIP_TRY(hipMemcpyAsync(f.size, size, (size_t)P * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(f.tot, 0, (size_t)B * sizeof(unsigned long long), st));
        HIP_TRY(hipMemsetAsync(f.clamp, 0, (size_t)B * sizeof(unsigned long long), st));
    }
    f.pblocks = (unsigned)(((size_t)P + kWaveThreads - 1) / kWaveThreads);
    k_wave_classify<Sized><<<f.pblocks, kWaveThreads, 0, st>>>(P, W, f.cur, f.tgt, f.wave, f.part, f.npart, f.mv, f.deg, f.d_ctl, f.size, C, f.traf,
                                                               f.tot, f.clamp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f.ctl, f.d_ctl, sizeof f.ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    f.n_mv = f.ctl[CTL_NMV];
    if (f.n_mv == 0) return KAO_OK;
    f.mblocks = (unsigned)((f.n_mv + kWaveThreads - 1) / kWaveThreads);
    k_wave_bound<Sized><<<f.mblocks, kWaveThreads, 0, st>>>(f.n_mv, k, f.part, f.npart, f.deg, f.khi, f.d_ctl, C, f.traf, f.tot, f.clamp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(f.ctl, f.d_ctl, sizeof f.ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return KAO_OK;
}

// The tail of every call: the winning order's waves (waveo, null when nothing moves) into wave[], wave[] read back, the results.
int wave_tail(WaveFront &f, int32_t P, const int32_t *waveo, int32_t best_waves, int32_t *wave, int32_t *n_waves, int32_t *lower_bound) {
    if (f.n_mv > 0) {
        k_wave_scatter<<<f.mblocks, kWaveThreads, 0, f.st>>>(f.n_mv, waveo, f.mv, f.wave);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(wave, f.wave, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToHost, f.st));
    HIP_TRY(hipStreamSynchronize(f.st));
    *n_waves = best_waves;
    *lower_bound = f.n_mv > 0 ? f.ctl[CTL_LB] : best_waves;
    return KAO_OK;
}

// The plain and the sized call after validation.
template <bool Sized>
int plan_waves(const char *fn, int32_t B, int32_t P, int32_t W, const uint16_t *current, const uint16_t *target, const uint64_t *size,
               uint64_t C, int32_t k, uint64_t seed, int32_t *wave, int32_t *n_waves, int32_t *lower_bound) {
    int rc = require_init();
    if (rc) return rc;
    *n_waves = 0;
    *lower_bound = 0;
    if (P == 0) return KAO_OK;
    WaveFront f;
    if ((rc = wave_front<Sized>(f, B, P, W, current, target, size, C, k))) return rc;
    if (f.n_mv == 0) return wave_tail(f, P, nullptr, f.ctl[CTL_CHANGED] ? 1 : 0, wave, n_waves, lower_bound);  // metadata-only partitions share wave 0
    const hipStream_t st = f.st;
    const int32_t n_mv = f.n_mv, wcap = f.ctl[CTL_WCAP];
    // per-order state: loads[B][wcap] (sized: only with a count cap), bytes[B][wcap] (sized), waveo[n_mv], three minkey rows [B]
    const bool counts = !Sized || k > 0;
    const size_t per_order = (size_t)B * wcap * ((counts ? 4 : 0) + (Sized ? 8 : 0)) + (size_t)n_mv * 4 + (size_t)3 * B * 8;
    const int n_ord = wave_orders(per_order);
    int32_t *d_loads = nullptr, *d_waveo, *d_nw, *d_flags;
    uint64_t *d_bytes = nullptr;
    unsigned long long *d_mk;
    if ((counts && (rc = f.m.alloc(&d_loads, (size_t)n_ord * B * wcap))) || (rc = f.m.alloc(&d_waveo, (size_t)n_ord * n_mv)) ||
        (rc = f.m.alloc(&d_mk, (size_t)3 * n_ord * B)) || (rc = f.m.alloc(&d_nw, (size_t)n_ord)) || (rc = f.m.alloc(&d_flags, 3)) ||
        (Sized && (rc = f.m.alloc(&d_bytes, (size_t)n_ord * B * wcap))))
        return rc;
    if (counts) HIP_TRY(hipMemsetAsync(d_loads, 0, (size_t)n_ord * B * wcap * sizeof(int32_t), st));
    if (Sized) HIP_TRY(hipMemsetAsync(d_bytes, 0, (size_t)n_ord * B * wcap * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(d_waveo, 0xFF, (size_t)n_ord * n_mv * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(d_mk, 0xFF, (size_t)2 * n_ord * B * sizeof(unsigned long long), st));  // rows of rounds 0 and 1
    HIP_TRY(hipMemsetAsync(d_nw, 0, (size_t)n_ord * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(d_flags, 0, 3 * sizeof(int32_t), st));
    const dim3 grid(f.mblocks, (unsigned)n_ord);
    k_wave_seed<<<grid, kWaveThreads, 0, st>>>(n_mv, B, seed, f.part, f.npart, f.mv, f.khi, d_mk);
    HIP_TRY(hipGetLastError());
    // every round places at least the lowest key of each order: n_mv rounds always suffice
    int32_t r = 0, left = 1;
    while (left) {
        if (r > n_mv) return fail(KAO_ERR_HIP, std::string(fn) + ": rounds did not finish");
        for (int i = 0; i < kWaveBatch; ++i, ++r)
            k_wave_round<Sized><<<grid, kWaveThreads, 0, st>>>(r, n_ord, n_mv, B, wcap, k, seed, f.part, f.npart, f.mv, f.khi, d_mk, d_loads, d_waveo,
                                                               d_nw, d_flags, f.d_ctl, C, f.traf, d_bytes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&left, d_flags + r % 3, sizeof left, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(f.ctl, f.d_ctl, sizeof f.ctl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (f.ctl[CTL_ERR]) return fail(KAO_ERR_HIP, std::string(fn) + ": a partition found no wave below the cap");
    }
    std::vector<int32_t> nw((size_t)n_ord);
    HIP_TRY(hipMemcpyAsync(nw.data(), d_nw, nw.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int best = (int)(std::min_element(nw.begin(), nw.end()) - nw.begin());  // first minimum: the lowest order
    return wave_tail(f, P, d_waveo + (size_t)best * n_mv, nw[(size_t)best], wave, n_waves, lower_bound);
}

// The state of the headroom call's orders (the layout is described above k_head_round) and the host's copy of their words.
struct HeadState {
    int n_ord = 0;
    uint64_t *capacity, *occ, *arr, *dep, *byt;
    int32_t *cnt, *waveo, *skipw, *n_done;
    unsigned long long *mk;
    HeadOrder *d_ord;
    std::vector<HeadOrder> ord;
};

// Uploads stored and capacity, allocates and clears the per-order state, and starts every order from occ = stored with the
// departures of the metadata-only partitions (k_head_dep0) waiting in wave 0.
int head_start(WaveFront &f, HeadState &h, int32_t B, int32_t P, int32_t W, const uint64_t *stored, const uint64_t *capacity) {
    const hipStream_t st = f.st;
    WaveBufs &m = f.m;
    uint64_t *d_stored;
    unsigned long long *d_dep0;
    int rc;
    if ((rc = m.alloc(&d_dep0, (size_t)B)) || (rc = m.alloc(&d_stored, (size_t)B)) || (rc = m.alloc(&h.capacity, (size_t)B))) return rc;
    HIP_TRY(hipMemcpyAsync(d_stored, stored, (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h.capacity, capacity, (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_dep0, 0, (size_t)B * sizeof(unsigned long long), st));
    k_head_dep0<<<f.pblocks, kWaveThreads, 0, st>>>(P, W, f.cur, f.tgt, f.size, d_dep0);
    HIP_TRY(hipGetLastError());
    // per-order state: occ, arr, dep, byt (8 bytes) and cnt (4) per broker, three minkey rows, waveo and skipw per slot
    const size_t per_order = (size_t)B * (4 * 8 + 4 + 3 * 8) + (size_t)f.n_mv * 8;
    h.n_ord = wave_orders(per_order);
    const size_t OB = (size_t)h.n_ord * B, OS = (size_t)h.n_ord * f.n_mv;
    if ((rc = m.alloc(&h.occ, OB)) || (rc = m.alloc(&h.arr, OB)) || (rc = m.alloc(&h.dep, OB)) || (rc = m.alloc(&h.byt, OB)) ||
        (rc = m.alloc(&h.cnt, OB)) || (rc = m.alloc(&h.mk, 3 * OB)) || (rc = m.alloc(&h.waveo, OS)) || (rc = m.alloc(&h.skipw, OS)) ||
        (rc = m.alloc(&h.d_ord, (size_t)h.n_ord)) || (rc = m.alloc(&h.n_done, 1)))
        return rc;
    HIP_TRY(hipMemsetAsync(h.arr, 0, OB * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(h.byt, 0, OB * sizeof(uint64_t), st));
    HIP_TRY(hipMemsetAsync(h.cnt, 0, OB * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(h.mk, 0xFF, 2 * OB * sizeof(unsigned long long), st));   // rows of rounds 0 and 1
    HIP_TRY(hipMemsetAsync(h.waveo, 0xFF, OS * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(h.skipw, 0xFF, OS * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(h.n_done, 0, sizeof(int32_t), st));
    h.ord.assign((size_t)h.n_ord, HeadOrder{0, 0, 0, 0, {0, 0, 0}, -1, -1, 0, ~0ull});
    HIP_TRY(hipMemcpyAsync(h.d_ord, h.ord.data(), h.ord.size() * sizeof(HeadOrder), hipMemcpyHostToDevice, st));
    k_head_init<<<dim3((unsigned)((B + kWaveThreads - 1) / kWaveThreads), (unsigned)h.n_ord), kWaveThreads, 0, st>>>(B, d_stored, d_dep0, h.occ, h.dep);
    HIP_TRY(hipGetLastError());
    return KAO_OK;
}

// Rounds and closes until every order has seen its idle wave, then the tally of the stuck slots; h.ord is read back.  *rounds =
// the round launches.
int head_rounds(const char *fn, WaveFront &f, HeadState &h, int32_t B, int32_t W, int32_t k, uint64_t C, uint64_t seed, int64_t *rounds) {
    const hipStream_t st = f.st;
    const int32_t n_mv = f.n_mv;
    const dim3 grid(f.mblocks, (unsigned)h.n_ord);
    // an order has at most n_mv + 2 waves (every wave but the first and the last takes a partition), a wave at most n_mv + 2
    // rounds (every round but its first and its last decides a slot)
    const int64_t max_rounds = ((int64_t)n_mv + 2) * ((int64_t)n_mv + 2);
    int64_t r = 0;
    int32_t n_done = 0;
    while (n_done < h.n_ord) {
        if (r > max_rounds) return fail(KAO_ERR_HIP, std::string(fn) + ": rounds did not finish");
        for (int i = 0; i < kWaveBatch; ++i, ++r) {
            const int32_t r3 = (int32_t)(r % 3);   // the kernels use the round number modulo 3 only
            k_head_round<<<grid, kWaveThreads, 0, st>>>(r3, h.n_ord, n_mv, B, W, k, C, seed, f.cur, f.tgt, f.size, h.capacity, f.part, f.npart, f.mv,
                                                        f.khi, f.traf, h.mk, h.occ, h.arr, h.dep, h.byt, h.cnt, h.waveo, h.skipw, h.d_ord);
            k_head_close<<<(unsigned)h.n_ord, kWaveThreads, 0, st>>>(r3, B, h.capacity, h.occ, h.arr, h.dep, h.byt, h.cnt, h.d_ord, h.n_done);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&n_done, h.n_done, sizeof n_done, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    k_head_tally<<<grid, kWaveThreads, 0, st>>>(n_mv, h.waveo, h.d_ord);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h.ord.data(), h.d_ord, h.ord.size() * sizeof(HeadOrder), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *rounds = r;
    return KAO_OK;
}

// The winning order: fewest stuck, then fewest waves, then the lowest order.  Its words go into st8[0] and st8[2..7].
int head_best(const HeadState &h, int64_t rounds, int64_t *st8) {
    int best = 0;
    for (int o = 1; o < h.n_ord; ++o)
        if (h.ord[(size_t)o].stuck < h.ord[(size_t)best].stuck ||
            (h.ord[(size_t)o].stuck == h.ord[(size_t)best].stuck && h.ord[(size_t)o].n_waves < h.ord[(size_t)best].n_waves))
            best = o;
    const HeadOrder &w = h.ord[(size_t)best];
    st8[0] = w.stuck;
    st8[2] = best;
    st8[3] = h.n_ord;
    st8[4] = rounds;
    if (w.mf_broker >= 0) {
        st8[5] = (int64_t)std::min<unsigned long long>(w.mf, (unsigned long long)INT64_MAX);
        st8[6] = w.mf_wave;
        st8[7] = w.mf_broker;
    }
    return best;
}

// The host pass over wave[]: the bytes of the stuck partitions (saturating), and whether wave 0 holds a metadata-only partition.
bool head_stuck_bytes_and_meta(int32_t P, int32_t W, const uint16_t *current, const uint16_t *target, const uint64_t *size, const int32_t *wave,
                               int64_t *stuck_bytes) {
    auto n_added = [&](int64_t p) {
        int na = 0;
        wave_each_added(current + p * W, target + p * W, W, [&](uint16_t) { ++na; });
        return na;
    };
    bool meta = false;   // metadata-only partitions share wave 0
    for (int64_t p = 0; p < P; ++p) {
        if (wave[p] == -2) {   // stuck bytes: one copy per added broker, each product below 2^62 (part of a broker's checked traffic)
            if (__builtin_add_overflow(*stuck_bytes, (int64_t)((uint64_t)n_added(p) * size[p]), stuck_bytes)) *stuck_bytes = INT64_MAX;
        } else if (wave[p] == 0 && !meta) {
            meta = n_added(p) == 0;
        }
    }
    return meta;
}

// The headroom call after validation.
int plan_headroom(const char *fn, int32_t B, int32_t P, int32_t W, const uint16_t *current, const uint16_t *target, const uint64_t *size,
                  const uint64_t *stored, const uint64_t *capacity, uint64_t C, int32_t k, uint64_t seed, int32_t *wave, int32_t *n_waves,
                  int32_t *lower_bound, int64_t *stats) {
    int rc = require_init();
    if (rc) return rc;
    *n_waves = 0;
    *lower_bound = 0;
    int64_t st8[8] = {0, 0, -1, 0, 0, -1, -1, -1};
    if (P == 0) {
        if (stats) std::copy(st8, st8 + 8, stats);
        return KAO_OK;
    }
    WaveFront f;
    if ((rc = wave_front<true>(f, B, P, W, current, target, size, C, k))) return rc;
    HeadState h;
    int32_t best_waves = 0;
    const int32_t *best_waveo = nullptr;
    if (f.n_mv > 0) {
        int64_t rounds = 0;
        if ((rc = head_start(f, h, B, P, W, stored, capacity)) || (rc = head_rounds(fn, f, h, B, W, k, C, seed, &rounds))) return rc;
        const int best = head_best(h, rounds, st8);
        best_waves = h.ord[(size_t)best].n_waves;
        best_waveo = h.waveo + (size_t)best * f.n_mv;
    }
    if ((rc = wave_tail(f, P, best_waveo, best_waves, wave, n_waves, lower_bound))) return rc;
    if (head_stuck_bytes_and_meta(P, W, current, target, size, wave, &st8[1])) *n_waves = std::max<int32_t>(*n_waves, 1);
    if (f.n_mv == 0) *lower_bound = *n_waves;
    if (stats) std::copy(st8, st8 + 8, stats);
    return KAO_OK;
}

}  // namespace

extern "C" int kao_plan_waves(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t *current, const uint16_t *target,
                              int32_t max_per_broker, uint64_t seed, int32_t *wave, int32_t *n_waves, int32_t *lower_bound) {
    int rc = validate_waves("kao_plan_waves", n_brokers, n_partitions, width, current, target, wave, n_waves, lower_bound);
    if (rc) return rc;
    if (max_per_broker < 1) return fail(KAO_ERR_INVALID, "kao_plan_waves: max_per_broker must be >= 1");
    return plan_waves<false>("kao_plan_waves", n_brokers, n_partitions, width, current, target, nullptr, 0, max_per_broker, seed, wave,
                             n_waves, lower_bound);
}

extern "C" int kao_plan_waves_sized(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t *current, const uint16_t *target,
                                    const uint64_t *size, uint64_t max_bytes_per_broker, int32_t max_per_broker, uint64_t seed, int32_t *wave,
                                    int32_t *n_waves, int32_t *lower_bound) {
    const char *fn = "kao_plan_waves_sized";
    int rc = validate_waves(fn, n_brokers, n_partitions, width, current, target, wave, n_waves, lower_bound);
    if (rc) return rc;
    if (!size) return fail(KAO_ERR_INVALID, "kao_plan_waves_sized: null size");
    if (max_per_broker < 0) return fail(KAO_ERR_INVALID, "kao_plan_waves_sized: max_per_broker must be >= 0");
    if (max_per_broker == 0 && max_bytes_per_broker == 0)
        return fail(KAO_ERR_INVALID, "kao_plan_waves_sized: max_bytes_per_broker and max_per_broker are both 0 (no cap)");
    if ((rc = validate_traffic(fn, n_brokers, n_partitions, width, current, target, size))) return rc;
    return plan_waves<true>(fn, n_brokers, n_partitions, width, current, target, size, max_bytes_per_broker, max_per_broker, seed, wave,
                            n_waves, lower_bound);
}

extern "C" int kao_plan_waves_headroom(int32_t n_brokers, int32_t n_partitions, int32_t width, const uint16_t *current, const uint16_t *target,
                                       const uint64_t *size, const uint64_t *stored, const uint64_t *capacity, uint64_t max_bytes_per_broker,
                                       int32_t max_per_broker, uint64_t seed, int32_t *wave, int32_t *n_waves, int32_t *lower_bound,
                                       int64_t stats[8]) {
    const char *fn = "kao_plan_waves_headroom";
    int rc = validate_waves(fn, n_brokers, n_partitions, width, current, target, wave, n_waves, lower_bound);
    if (rc) return rc;
    if (!size) return fail(KAO_ERR_INVALID, "kao_plan_waves_headroom: null size");
    if (!stored) return fail(KAO_ERR_INVALID, "kao_plan_waves_headroom: null stored");
    if (!capacity) return fail(KAO_ERR_INVALID, "kao_plan_waves_headroom: null capacity");
    if (max_per_broker < 0) return fail(KAO_ERR_INVALID, "kao_plan_waves_headroom: max_per_broker must be >= 0");
    if ((rc = validate_traffic(fn, n_brokers, n_partitions, width, current, target, size))) return rc;
    if ((rc = validate_stored(fn, n_brokers, n_partitions, width, current, target, size, stored))) return rc;
    return plan_headroom(fn, n_brokers, n_partitions, width, current, target, size, stored, capacity, max_bytes_per_broker, max_per_broker,
                         seed, wave, n_waves, lower_bound, stats);
}
