// kao_logdirs.hip -- kao_balance_logdirs and kao_place_logdirs.  kao_balance_logdirs: replica moves between the log dirs of ONE broker that lower the peak of the bytes a dir
// stores, every broker of the call at once.  Kernels and the C entry point.
//
// Broker b owns the dirs dir_start[b] .. dir_start[b+1]-1 (at most KAO_LOGDIRS_MAX_DIRS), dir d carries base[d] bytes that never move,
// replica r sits in dir[r] with size[r] bytes, L(d) = base[d] + the sizes of its replicas.  A move takes r to another dir of the same
// broker: the brokers are independent sub-problems, and each is the descent of section 4k with the pairing of section 4m:
//   k_ld_count, k_bucket_offsets (kao_plan_dev.h), k_ld_scatter   the replicas bucketed by broker (count, prefix sum + largest bucket, scatter)
//   k_ld_solve   ONE WORKGROUP PER BROKER, all brokers in one launch: every round, then the bound, then the row of per_broker
// THE FRAME of a broker's workgroup is written once and shared by k_ld_solve and k_ld_place (below): its static LDS is one LdLds, its
// broker one LdBroker.  ld_begin: a broker without dirs gets its row at once; else base (and cap) into the loads, one pass over the
// bucket that adds the residents' sizes and hands a homeless replica to the caller, the peak before and the statistics of the bound.
// ld_end: the peak after, the replicas that left their input dir, the bound and its proof, the row of per_broker (its columns per
// kernel: kLdRow) and the call's counters.  Between the two stands what is the kernel's own: the rounds (ld_rounds, ld_xchg_rounds)
// for k_ld_solve; sort, greedy pass and, when asked, the rounds for k_ld_place.  On the host LdCall is the same frame around the
// launch: open (arena, uploads, buckets, lane count, common arguments), finish (read-back and outputs).
// A ROUND uses the loads as they stand at its start and has four parts with a barrier after each:
//   RANK     the lanes below n rank the broker's n dirs by L descending (ties: index ascending) by all pairs out of LDS;
//   PROPOSE  every replica with size > 0 (n >= 2) on a of rank q takes c1 = order[n-1-q] when q < n-1-q and proposes a -> c1 iff
//            L(c1) + size + min_gain < L(a); otherwise, when q >= 1, c2 = order[n-1] under the same test.  It bids
//            key = q << 48 | (0xFFFF - code(size)) << 32 | r into the minkey word of a and of its destination (LDS atomicMin, skipped
//            when the word is already lower).  The barrier is __syncthreads_or("I proposed"): the end test;
//   DECIDE   a proposal wins iff both words hold its key; only minkey words are read, only the replica's own flag is written;
//   APPLY    winners store L(a) -= size, L(c) += size and their dir (no two winners share a dir), every proposer clears its two words.
// No lane reads a load in the part in which another lane can write it: the snapshot rule of section 4k.  LDS per workgroup: load and
// minkey u64[64], rank and order u8[64], a few words of reduction: under 2 KiB, static, so many brokers share a compute unit.  The
// round state of a replica (key, destination | won) sits in HBM / L2 at the replica's place in its bucket and is read back by the lane
// that wrote it; its dir is dir[r].
// The BOUND of a broker, valid for every placement of its replicas, integers only: the maximum of (0) the largest size + the smallest
// base, (1) ceil(sum of L / n), (2) the largest base.
//
// kao_place_logdirs shares the file: replica r belongs to broker[r] and is a resident (dir[r] >= 0) or homeless
// (dir[r] == -1: a replica that a plan brings to the broker, or one of a dir that is being emptied).  The buckets are keyed by
// broker[r], through the same three passes, which also count the homeless replicas of a broker and the largest such count.
//   k_ld_place   ONE WORKGROUP PER BROKER: the loads F of the residents into LDS, the homeless replicas compacted into (~size, r)
//                entries (both in the pass of ld_begin) and sorted (size descending, then r ascending) by a bitonic network, in
//                dynamic LDS up to kLdSortLds entries a broker and else in the bucket's own scratch in global memory; wavefront 0
//                then takes them one by one, each to the dir with the lowest load at that moment (ties: the lowest index); with
//                move_residents the rounds above follow (ld_rounds, the one copy of the loop that k_ld_solve calls too); then
//                ld_end: the bound and the row of per_broker.
// Its bound: M = the replicas that may change dir (the homeless; all with move_residents), F' = the fixed loads (F; base with
// move_residents): the maximum of (0) the largest size in M + the smallest F', (1) ceil((sum of base + sum of size) / n), (2) the largest F'.
//
// kao_balance_logdirs_exchange is k_ld_solve<false, true>: the rounds above, and when a round has no move
// proposal an EXCHANGE round in its place (ld_rounds<Cap, true>).  Before the rounds the workgroup sorts the bucket once into PI
// (size descending, then r ascending; ld_sort, the network of k_ld_place) and keeps one bitmask over the positions of PI per dir: bit
// p of mask[d] is set iff the replica at position p sits in d.  The lanes then stride over the positions of PI, not over the bucket:
// list[] is PI's r, and key[], dst[] and partner[] are by position.  EXCHANGE PROPOSE of the replica x at position p, on a of rank q:
// for the dirs c of the ranks n-1 .. q+1, D = L(a) - L(c) > 0, g = the first position whose size s has 2 s <= 2 size[x] - D (a binary
// search in PI), y_lo = the next set bit of mask[c] from g, y_hi = the last one before g (word scans); the better passing candidate of
// the first dir that has one is bid with key q << 48 | (0xFFFF - code(delta)) << 32 | x.  DECIDE is the one above.  APPLY: only a
// winner works; it alone touches the loads and the mask rows of a and c (winners share no dir) and stores dir[x] and dir[y]: y is no
// winner, and no lane reads the dir of a replica other than a winner's own in this part; the lanes below n clear the minkey words.
// PI and the masks sit in dynamic LDS while the call's largest bucket holds at most kLdSortLds replicas and 12 bytes a replica + 8
// bytes a mask word fit kLdXchgLds for that bucket and the most dirs of a broker, else in global memory at the bucket's place
// (kao_logdirs_test_exchange forces either).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "kao_host.h"
#include "kao_plan_dev.h"   // descent_gains, descent_bid, wave_bytes_code

namespace {

constexpr int kLdThreads = 256;          // the passes over replicas
constexpr int kLdSoloSmall = 256;        // lanes of a broker's workgroup while the largest bucket holds at most kLdSmallBucket replicas
constexpr int kLdSoloLarge = 1024;       // (the kFoSoloSmall / kFoSoloLarge rule of kao_failover_dev.h)
constexpr int kLdSmallBucket = 1024;
constexpr int kLdMaxDirs = KAO_LOGDIRS_MAX_DIRS;
constexpr int kLdMaxReplicas = 4000000;
constexpr int kLdHardRounds = 1 << 26;   // no descent gets here; a guard against an endless loop
constexpr u64 kLdNoKey = ~0ull;
constexpr int kLdWon = 0x80;             // flag in dst[]: this round's proposal won (a destination is below 64)
constexpr int kLdSortLds = 4096;         // kao_place_logdirs: homeless replicas of one broker sorted in dynamic LDS (12 bytes each: 48 KiB of the 64 KiB a launch gets unasked)
constexpr int kLdXchgLds = 60 << 10;      // kao_balance_logdirs_exchange: dynamic LDS for PI and the masks of one broker; with the static 1.5 KiB a workgroup stays under the
                                         // 64 KiB that a launch gets unasked, and two such workgroups share the 160 KiB of a compute unit
enum { LC_PEAK0 = 0, LC_PEAK1, LC_NMOVED, LC_BYTES, LC_BROKERS, LC_ROUNDS, LC_MOVES, LC_PROPS, LC_MORE, LC_PROVEN, LC_MAXROUNDS, LC_ERR, LC_MAXN, LC_MAXH /* = LC_MAXN + 1 */,
       LC_NPLACED, LC_BPLACED, LC_PLACERS, LC_XROUNDS, LC_XCH, LC_XPROPS, LC_XLOWER, LC_N = 24 };
enum { LS_PEAK0 = 0, LS_PEAK1, LS_MAXSIZE, LS_MINBASE, LS_MAXBASE, LS_TOTAL, LS_NMOVED, LS_BYTES, LS_MOVES, LS_PROPS, LS_MINF, LS_HBYTES, LS_PEAK0DEN /* Cap */, LS_XCH, LS_XPROPS,
       LS_N = 16 };
typedef unsigned __int128 u128;
static_assert(kLdMaxDirs == 64, "a wavefront ranks the dirs of a broker; a destination and kLdWon share a byte");

struct LdNet {   // one call; every pointer is device memory
    int max_rounds;
    u64 min_gain;
    const int32_t *dir_start;   // [B + 1]
    const u64 *base;            // [n_dirs]
    const u64 *size;            // [R]
    int32_t *dir;               // [R] rewritten by the winners
    const int32_t *dir0;        // [R] the input
    const int32_t *cnt, *start, *list;   // [B], [B], [R]: the brokers' buckets of replica indices
    u64 *key;                   // [R] by place in the bucket: key of this round's proposal, kLdNoKey = none
    uint8_t *dst;               // [R] by place in the bucket: its destination (index inside the broker) | kLdWon
    u64 *per_broker;            // [6B]; [8B] for k_ld_place
    u64 *ctl;                   // [LC_N]
    // k_ld_place alone
    int move_residents, sort_lds, sort_cap;   // the rounds follow PLACE; the sort runs in dynamic LDS of sort_cap entries (else in the bucket)
    const int32_t *hcnt;        // [B] homeless replicas of a broker
    uint32_t *sr;               // [R] by place in the bucket: the r of a sort entry on the global path (its size sits in key[])
    // the capacity calls alone (Cap; per_broker is then [10B], [12B] for k_ld_place)
    const u64 *cap;             // [n_dirs] bytes of disk behind a dir, >= 1
};
struct LdNetX : LdNet {         // the exchange call (X; per_broker is then [8B]): sr is PI's r on the global path.  A type of its own: the other kernels keep their arguments
    int x_lds, x_cap, x_mcap;   // PI and the masks sit in dynamic LDS of x_cap entries and x_mcap mask words (else at the bucket's place)
    u64 *xs;                    // [R] by place in the bucket: PI's sizes on the global path
    u64 *xm;                    // [R + n_dirs] the masks of broker b on the global path, from word start[b] + dir_start[b]
    uint32_t *xp;               // [R] by position in PI: the position of the partner of this round's proposal
};

// The static LDS of a broker's workgroup: the loads (Cap: the pairs {load, cap}), the minkey words, the LS_* words, the ranks of the dirs and the dirs by rank.
template <bool Cap>
struct LdLds {
    alignas(16) u64 load[(Cap ? 2 : 1) * kLdMaxDirs];   // 16 bytes: RANK reads two loads (Cap: one {load, cap}) with one 128-bit LDS read
    u64 mk[kLdMaxDirs], sh[LS_N];
    uint8_t rank[kLdMaxDirs], order[kLdMaxDirs];
};
// The broker of a workgroup: its dirs ds .. ds + nd - 1, its bucket (nr replicas, h of them homeless) with the round state at the bucket's place `at`, its row of per_broker.
struct LdBroker {
    int ds, nd, nr, h, at;
    const int32_t *list;
    u64 *key;
    uint8_t *dst;
    u64 *o;
    u64 fixed;   // Cap: F(d), the load of dir d with its residents alone, in lane d of wavefront 0
};
// A row of per_broker: {peak before, peak after, bound}, with Cap the three as fractions {peak, its cap, peak, its cap, bound num, den}, then {placed, bytes
// placed} from column `placed`, {moved, bytes moved, rounds} from `moved`, {exchange rounds, exchanges} from `xch`, the proof at `proof`; -1 = not in the row.
struct LdRow {
    int w, placed, moved, xch, proof;
};
template <bool Cap, bool X, bool Place>
constexpr LdRow kLdRow = Place ? (Cap ? LdRow{12, 6, 8, -1, 11} : LdRow{8, 3, 5, -1, -1})   // k_ld_place
                               : X ? LdRow{8, -1, 3, 6, -1} : Cap ? LdRow{10, -1, 6, -1, 9} : LdRow{6, -1, 3, -1, -1};   // k_ld_solve

// ---- Cap: the descent by utilisation u(d) = L(d) / cap(d) -------------------------------------------------------
// The loads of a broker sit in LDS as load[d] (Cap = false) or as the pairs {load, cap} = load[2d], load[2d + 1] (Cap = true): one
// 128-bit read brings both.  No quotient is formed: x / cx is above y / cy iff x * cy > y * cx in 128 bits (loads < 2^62, caps < 2^62).
template <bool Cap>
__device__ __forceinline__ u64 &ld_load(u64 *load, int d) { return load[Cap ? 2 * d : d]; }
struct LdPair {
    u64 l, c;
};
__device__ __forceinline__ LdPair ld_pair(const u64 *load, int d) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(load + 2 * d);
    return {v.x, v.y};
}
// (L(c) + w + min_gain) * cap(a) < L(a) * cap(c); a 64-bit sum that overflows does not pass (L(c) + w stays below 2^63)
__device__ __forceinline__ bool ld_gains_cap(LdPair a, LdPair c, u64 w, u64 min_gain) {
    u64 s;
    if (__builtin_add_overflow(c.l + w, min_gain, &s)) return false;
    return (u128)s * a.c < (u128)a.l * c.c;
}
// Over the 64 lanes of a wavefront, all active: the highest (Max) or the lowest fraction num / den, ties to the lowest idx (the idx
// are distinct); every lane ends with the same {num, den, idx}.
template <bool Max>
__device__ __forceinline__ void ld_frac_reduce(u64 &num, u64 &den, int &idx) {
    for (int x = 32; x >= 1; x >>= 1) {
        const u64 on = __shfl_xor(num, x), od = __shfl_xor(den, x);
        const int oi = __shfl_xor(idx, x);
        const u128 theirs = (u128)on * den, ours = (u128)num * od;
        const bool take = (Max ? theirs > ours : theirs < ours) || (theirs == ours && oi < idx);
        num = take ? on : num;
        den = take ? od : den;
        idx = take ? oi : idx;
    }
}
// the sum over the 64 lanes, cut at 2^62 (every v is at most 2^62)
__device__ __forceinline__ u64 ld_wave_sum(u64 v) {
    for (int x = 32; x >= 1; x >>= 1) v = min(v + __shfl_xor(v, x), 1ull << 62);
    return v;
}
// The peak after, the bound and the proof of one broker (include/kao.h: kao_balance_logdirs_capacity), by the 64 lanes of wavefront
// 0: lane d < nd brings L = its load, c = its capacity, f = its fixed load F'(d); mx = the largest size in M, any = M is not empty.
// o[0..1] = the peak {L, cap}, o[2..3] = the bound {num, den}; returns the proof (0 gap, 1 bound met, 2 integrality test only).
__device__ __forceinline__ int ld_cap_bound(int nd, u64 L, u64 c, u64 f, u64 mx, bool any, u64 *o) {
    const int lane = threadIdx.x;
    const bool v = lane < nd;
    u64 pn = v ? L : 0, pd = v ? c : 1;
    int pi = lane;
    ld_frac_reduce<true>(pn, pd, pi);
    u64 bn = 0, bd = 1;                       // term (0): the lowest {F'(d) + mx, cap(d)}; a lane past nd sorts after every dir
    if (any) {
        bn = v ? f + mx : kLdNoKey;
        bd = v ? c : 1;
        int bi = lane;
        ld_frac_reduce<false>(bn, bd, bi);
    }
    const u64 total = ld_wave_sum(v ? L : 0), fsum = ld_wave_sum(v ? f : 0), csum = ld_wave_sum(v ? c : 0);   // below 2^62: not cut
    if ((u128)total * bd > (u128)bn * csum) { bn = total; bd = csum; }   // term (1): sum of F' + sum over M = the sum of the loads
    u64 tn = v ? f : 0, td = v ? c : 1;       // term (2)
    int ti = lane;
    ld_frac_reduce<true>(tn, td, ti);
    if ((u128)tn * bd > (u128)bn * td) { bn = tn; bd = td; }
    if (lane == 0) { o[0] = pn; o[1] = pd; o[2] = bn; o[3] = bd; }
    if ((u128)pn * bd == (u128)bn * pd) return 1;
    // the integrality test: a dir strictly below the peak pn / pd holds at most ceil(pn * cap(d) / pd) - 1 bytes, so room(d) of them
    // for M; when the rooms sum to less than M's bytes no outcome is strictly below the peak everywhere.  (pn >= 1: the peak is above the bound.)
    const u64 msum = total - fsum;
    u64 room = 0;
    if (v) {
        const u128 q = ((u128)pn * c + pd - 1) / pd - 1;
        if (q > f) room = q - f > msum ? msum : (u64)(q - f);
    }
    return ld_wave_sum(room) < msum ? 2 : 0;
}

// ---- the buckets --------------------------------------------------------------------------------------------------------------------
// The broker of replica r is map[idx[r]] (kao_balance_logdirs: the broker of its dir), or idx[r] when map is null (kao_place_logdirs:
// broker[r]); hcnt, when not null, counts the replicas with dir[r] < 0 beside.
__global__ void k_ld_count(int R, const int32_t *__restrict__ idx, const int32_t *__restrict__ map, const int32_t *__restrict__ dir, int32_t *__restrict__ cnt,
                           int32_t *__restrict__ hcnt) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int b = map ? map[idx[r]] : idx[r];
    atomicAdd(&cnt[b], 1);
    if (hcnt && dir[r] < 0) atomicAdd(&hcnt[b], 1);
}

// (between the two: k_bucket_offsets of kao_plan_dev.h, whose maxima, the largest cnt and the largest hcnt, go to ctl[LC_MAXN] and ctl[LC_MAXH])
// the order inside a bucket does not reach the result: the keys carry r
__global__ void k_ld_scatter(int R, const int32_t *__restrict__ idx, const int32_t *__restrict__ map, const int32_t *__restrict__ start,
                             int32_t *__restrict__ fill, int32_t *__restrict__ list) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int b = map ? map[idx[r]] : idx[r];
    list[start[b] + atomicAdd(&fill[b], 1)] = r;
}

// ---- the rounds of one broker (RANK / PROPOSE / DECIDE / APPLY of the head of this file), called by every lane of its workgroup with the
// loads in place, mk[] at kLdNoKey and every replica of the bucket in a dir.  rounds and more are the workgroup's, props and moves this lane's.
struct LdTally {
    int rounds = 0, more = 0;
    u64 props = 0, moves = 0;
};
struct LdTallyX : LdTally {          // X: rounds, props and moves count both kinds
    int xrounds = 0, xlowered = 0;   // the workgroup's exchange rounds; one of them lowered the peak
    u64 xprops = 0, xch = 0;         // this lane's exchange proposals and exchanges
};
// X: PI and the masks of the broker: ps[p] the size at position p (descending), bit p & 63 of mask[d * words + (p >> 6)] = the replica
// at position p sits in dir d, partner[p] the position of the partner of p's proposal.  list[] is then PI's r.
struct LdXchg {
    const u64 *ps = nullptr;
    u64 *mask = nullptr;
    uint32_t *partner = nullptr;
    int words = 0;
};
// the first set bit of the mask row m at a position >= g, the last one at a position < g; -1 without one (no bit is set past nr)
__device__ __forceinline__ int ld_next_bit(const u64 *m, int words, int g, int nr) {
    if (g >= nr) return -1;
    int wi = g >> 6;
    u64 v = m[wi] & (~0ull << (g & 63));
    while (!v) {
        if (++wi >= words) return -1;
        v = m[wi];
    }
    return wi * 64 + __ffsll((unsigned long long)v) - 1;
}
__device__ __forceinline__ int ld_prev_bit(const u64 *m, int g) {
    if (g <= 0) return -1;
    const int h = g - 1;
    int wi = h >> 6;
    u64 v = m[wi] & (~0ull >> (63 - (h & 63)));
    while (!v) {
        if (--wi < 0) return -1;
        v = m[wi];
    }
    return wi * 64 + 63 - __clzll((long long)v);
}
// one candidate of an exchange: y of size sy for x of size w across the gap D; passes iff sy > 0, delta = w - sy > 0 and
// delta + min_gain < D (delta < D and D - delta > min_gain: no overflow); far = |2 delta - D|
__device__ __forceinline__ bool ld_xchg_passes(u64 w, u64 sy, u64 D, u64 min_gain, u64 &delta, u64 &far) {
    if (!sy || w <= sy) return false;
    delta = w - sy;
    if (delta >= D || D - delta <= min_gain) return false;
    far = 2 * delta > D ? 2 * delta - D : D - 2 * delta;
    return true;
}
template <bool Cap, bool X = false>
__device__ __forceinline__ std::conditional_t<X, LdTallyX, LdTally> ld_rounds(const LdNet &n, const LdBroker &br, LdLds<Cap> &s, const LdXchg x = LdXchg()) {
    static_assert(!(Cap && X), "exchange rounds are by bytes");
    const int tid = threadIdx.x, NT = blockDim.x, ds = br.ds, nd = br.nd, nr = br.nr;
    const int32_t *list = br.list;
    u64 *key = br.key, *load = s.load, *mk = s.mk;
    uint8_t *dst = br.dst, *rank = s.rank, *order = s.order;
    std::conditional_t<X, LdTallyX, LdTally> t;
    [[maybe_unused]] u64 peak = 0;         // X: the peak at the start of the round before
    [[maybe_unused]] bool was_x = false;   // X: that round was an exchange round
    for (;;) {
        if (tid < nd) {   // RANK
            int q = 0;
            if constexpr (Cap) {   // by u descending: all pairs by products
                const LdPair me = ld_pair(load, tid);
                for (int j = 0; j < nd; ++j) {
                    const LdPair x = ld_pair(load, j);
                    const u128 theirs = (u128)x.l * me.c, ours = (u128)me.l * x.c;
                    q += (theirs > ours || (theirs == ours && j < tid)) ? 1 : 0;
                }
            } else {
                const u64 mine = load[tid];
                for (int j = 0; j < nd; ++j) {
                    const u64 x = load[j];
                    q += (x > mine || (x == mine && j < tid)) ? 1 : 0;
                }
            }
            rank[tid] = (uint8_t)q;   // ranks are a permutation: q < nd
            order[q] = (uint8_t)tid;
        }
        __syncthreads();
        if constexpr (X) {   // the peak is the load of the dir of rank 0
            const u64 now = load[order[0]];
            if (was_x && now < peak) t.xlowered = 1;
            peak = now;
        }
        int mine = 0;
        for (int q = tid; q < nr; q += NT) {   // PROPOSE
            const int r = list[q];
            const u64 w = n.size[r];
            u64 k = kLdNoKey;
            if (w && nd >= 2) {
                const int a = n.dir[r] - ds, ra = rank[a];
                int c = -1;
                if constexpr (Cap) {   // c1, then the walk over the ranks n-1 .. q+1: the first dir that passes (a fuller but larger dir can pass where the emptiest does not)
                    const LdPair pa = ld_pair(load, a);
                    const int p1 = nd - 1 - ra;
                    if (ra < p1) {
                        const int c1 = order[p1];
                        if (ld_gains_cap(pa, ld_pair(load, c1), w, n.min_gain)) c = c1;
                    }
                    for (int p = nd - 1; c < 0 && p > ra; --p) {
                        if (p == p1) continue;   // c1, which did not pass
                        const int cw = order[p];
                        if (ld_gains_cap(pa, ld_pair(load, cw), w, n.min_gain)) c = cw;
                    }
                } else {
                    const u64 la = load[a];
                    if (ra < nd - 1 - ra) {
                        const int c1 = order[nd - 1 - ra];
                        if (descent_gains(la, load[c1], w, n.min_gain)) c = c1;
                    }
                    if (c < 0 && ra >= 1) {
                        const int c2 = order[nd - 1];   // (a itself when a is the lightest: it does not pass)
                        if (descent_gains(la, load[c2], w, n.min_gain)) c = c2;
                    }
                }
                if (c >= 0) {
                    k = (u64)(uint32_t)ra << 48 | (u64)(0xFFFFu - wave_bytes_code(w)) << 32 | (u64)(uint32_t)r;
                    dst[q] = (uint8_t)c;
                    descent_bid<__HIP_MEMORY_SCOPE_WORKGROUP>(&mk[a], k);
                    descent_bid<__HIP_MEMORY_SCOPE_WORKGROUP>(&mk[c], k);
                    ++mine;
                }
            }
            key[q] = k;   // key[q], dst[q] and dir[r] are read back by this lane alone
        }
        [[maybe_unused]] bool isx = false;
        if constexpr (X) {
            if (!__syncthreads_or(mine)) {   // no move proposal: EXCHANGE PROPOSE (every key[q] is kLdNoKey and no minkey word was bid)
                isx = true;
                for (int q = tid; q < nr; q += NT) {
                    const u64 w = x.ps[q];
                    u64 k = kLdNoKey;
                    if (w) {
                        const int r = list[q], a = n.dir[r] - ds, ra = rank[a];
                        const u64 la = load[a];
                        for (int p = nd - 1; p > ra && k == kLdNoKey; --p) {   // the lightest dir first
                            const int c = order[p];
                            const u64 lc = load[c];
                            if (la <= lc || la - lc <= n.min_gain) continue;   // D <= 0; D <= min_gain: no delta > 0 has delta + min_gain < D
                            const u64 D = la - lc;
                            const int64_t T = 2 * (int64_t)w - (int64_t)D;     // every term below 2^63
                            int g = 0, hi = nr;                                // g = the sizes s with 2 s > T: they come first in PI
                            while (g < hi) {
                                const int mid = (g + hi) >> 1;
                                if ((int64_t)(2 * x.ps[mid]) > T) g = mid + 1;
                                else hi = mid;
                            }
                            const u64 *m = x.mask + (size_t)c * x.words;
                            const int jl = ld_next_bit(m, x.words, g, nr), jh = ld_prev_bit(m, g);
                            int j = -1;
                            u64 delta = 0, far = 0, dh = 0, fh = 0;
                            if (jl >= 0 && ld_xchg_passes(w, x.ps[jl], D, n.min_gain, delta, far)) j = jl;
                            if (jh >= 0 && ld_xchg_passes(w, x.ps[jh], D, n.min_gain, dh, fh) && (j < 0 || fh < far)) {   // a tie goes to y_lo
                                j = jh;
                                delta = dh;
                            }
                            if (j >= 0) {
                                k = (u64)(uint32_t)ra << 48 | (u64)(0xFFFFu - wave_bytes_code(delta)) << 32 | (u64)(uint32_t)r;
                                dst[q] = (uint8_t)c;
                                x.partner[q] = (uint32_t)j;
                                descent_bid<__HIP_MEMORY_SCOPE_WORKGROUP>(&mk[a], k);
                                descent_bid<__HIP_MEMORY_SCOPE_WORKGROUP>(&mk[c], k);
                                ++mine;
                            }
                        }
                    }
                    key[q] = k;
                }
                if (!__syncthreads_or(mine)) break;
            }
        } else if (!__syncthreads_or(mine)) break;
        if ((n.max_rounds > 0 && t.rounds >= n.max_rounds) || t.rounds >= kLdHardRounds) { t.more = 1; break; }
        ++t.rounds;
        t.props += (u64)mine;
        if constexpr (X) {
            was_x = isx;
            if (isx) { ++t.xrounds; t.xprops += (u64)mine; }
        }
        for (int q = tid; q < nr; q += NT) {   // DECIDE
            const u64 k = key[q];
            if (k == kLdNoKey) continue;
            const int c = dst[q];
            if (mk[n.dir[list[q]] - ds] == k && mk[c] == k) dst[q] = (uint8_t)(c | kLdWon);
        }
        __syncthreads();
        if constexpr (X) {   // APPLY by the winners alone: no other lane writes a winner's dir[x] (its partner y never wins), the mask rows of a and c are its own
            if (tid < nd) mk[tid] = kLdNoKey;   // (no lane reads a minkey word in this part)
            for (int q = tid; q < nr; q += NT) {
                if (key[q] == kLdNoKey || !(dst[q] & kLdWon)) continue;
                const int r = list[q], c = dst[q] & (kLdWon - 1), a = n.dir[r] - ds;
                u64 *ma = x.mask + (size_t)a * x.words, *mc = x.mask + (size_t)c * x.words;
                u64 d = x.ps[q];
                ma[q >> 6] &= ~(1ull << (q & 63));
                mc[q >> 6] |= 1ull << (q & 63);
                if (isx) {
                    const int j = (int)x.partner[q];
                    d -= x.ps[j];
                    n.dir[list[j]] = ds + a;
                    mc[j >> 6] &= ~(1ull << (j & 63));
                    ma[j >> 6] |= 1ull << (j & 63);
                    ++t.xch;
                }
                load[a] -= d;
                load[c] += d;
                n.dir[r] = ds + c;
                ++t.moves;
            }
            __syncthreads();
            continue;
        }
        for (int q = tid; q < nr; q += NT) {   // APPLY
            if (key[q] == kLdNoKey) continue;
            const int r = list[q], s = dst[q], c = s & (kLdWon - 1), a = n.dir[r] - ds;
            if (s & kLdWon) {   // no other winner touches a or c
                const u64 w = n.size[r];
                ld_load<Cap>(load, a) -= w;
                ld_load<Cap>(load, c) += w;
                n.dir[r] = ds + c;
                ++t.moves;
            }
            mk[a] = kLdNoKey;
            mk[c] = kLdNoKey;
        }
        __syncthreads();
    }
    return t;
}

template <class K, class I>
__device__ __forceinline__ void ld_sort(K sk, I sr, int h);   // below, with k_ld_place

// ---- the rounds with exchanges of one broker: PI into ps[] / pr[] (nr entries each), the masks into mask[]
// (nd rows of nr / 64 + 1 words), then ld_rounds<false, true> over the positions of PI.  Called by every lane of the workgroup.
__device__ __forceinline__ LdTallyX ld_xchg_rounds(const LdNet &n, const LdBroker &br, LdLds<false> &s, u64 *ps, u64 *mask, uint32_t *pr, uint32_t *partner) {
    const int tid = threadIdx.x, NT = blockDim.x, ds = br.ds, nd = br.nd, nr = br.nr, words = nr / 64 + 1;
    for (int q = tid; q < nr; q += NT) {   // the sort's entries (~size, r), in any order
        const int r = br.list[q];
        ps[q] = ~n.size[r];
        pr[q] = (uint32_t)r;
    }
    for (int i = tid; i < nd * words; i += NT) mask[i] = 0;
    __syncthreads();
    if (nr >= 2) ld_sort(ps, pr, nr);
    for (int q0 = tid & ~63; q0 < nr; q0 += NT) {   // 64 positions a wavefront and step: they share a mask word, one lane of each dir stores the dir's bits
        const int q = q0 + (tid & 63);
        int d = -1;
        if (q < nr) {
            ps[q] = ~ps[q];
            d = n.dir[pr[q]] - ds;
        }
        for (u64 left = __ballot(d >= 0); left;) {
            const int d0 = __shfl(d, __ffsll((unsigned long long)left) - 1);
            const u64 same = __ballot(d == d0);
            if ((tid & 63) == __ffsll((unsigned long long)same) - 1) mask[(size_t)d0 * words + (q0 >> 6)] = same;
            left &= ~same;
        }
    }
    // (the barrier of the first RANK comes before any read of ps[] and mask[])
    LdXchg x;
    x.ps = ps; x.mask = mask; x.partner = partner; x.words = words;
    LdBroker pi = br;   // the rounds stride over the positions of PI
    pi.list = reinterpret_cast<const int32_t *>(pr);
    return ld_rounds<false, true>(n, pi, s, x);
}

// ---- the frame of one broker: what k_ld_solve and k_ld_place do before and after the parts of their own ------------------------------
// BEGIN, by every lane: the broker of this workgroup into br.  Without a dir its row is written here (zeros, the fractions 0 / 1,
// nothing to prove) and the answer is true: the workgroup is done.  Else the LS_* words are cleared, base and cap go into the loads,
// mk[] to kLdNoKey, and one pass over the bucket adds a resident's size to the load of its dir and, with Place, hands a homeless
// replica to homeless(r, size) and sums LS_HBYTES; LS_MAXSIZE = the largest size of the replicas that may change dir.  Then the peak
// before: Cap: the fullest dir as a fraction by wavefront 0, with F(d) into br.fixed; else LS_PEAK0 and LS_TOTAL, with Place LS_MINF,
// beside the smallest and the largest base.  No barrier closes it: the caller's next one does.
template <bool Cap, bool X, bool Place, class Homeless>
__device__ __forceinline__ bool ld_begin(const LdNet &n, LdLds<Cap> &s, LdBroker &br, Homeless homeless) {
    constexpr LdRow row = kLdRow<Cap, X, Place>;
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int ds = n.dir_start[b], nd = n.dir_start[b + 1] - ds, nr = n.cnt[b], at = n.start[b];
    u64 *sh = s.sh, *o = n.per_broker + row.w * (size_t)b;
    br = {ds, nd, nr, Place ? n.hcnt[b] : 0, at, n.list + at, n.key + at, n.dst + at, o, 0};
    if (nd == 0) {   // no dir, so no replica
        if (tid == 0) {
            for (int i = 0; i < row.w; ++i) o[i] = 0;
            if constexpr (Cap) { o[1] = o[3] = o[5] = 1; o[row.proof] = 1; }
            atomicAdd(&n.ctl[LC_PROVEN], 1ull);
        }
        return true;
    }
    if (tid < LS_N) sh[tid] = (tid == LS_MINBASE || tid == LS_MINF) ? kLdNoKey : 0;
    if (tid < nd) {
        ld_load<Cap>(s.load, tid) = n.base[ds + tid];
        if constexpr (Cap) s.load[2 * tid + 1] = n.cap[ds + tid];
        s.mk[tid] = kLdNoKey;
    }
    __syncthreads();
    {
        u64 mx = 0, hb = 0;
        for (int q = tid; q < nr; q += NT) {
            const int r = br.list[q], d = n.dir[r];
            const u64 w = n.size[r];
            if (!Place || d >= 0) {
                if (w) atomicAdd(&ld_load<Cap>(s.load, d - ds), w);
                if (!Place || n.move_residents) mx = max(mx, w);
            } else {
                homeless(r, w);
                hb += w;
                mx = max(mx, w);
            }
        }
        if (mx) atomicMax(&sh[LS_MAXSIZE], mx);
        if (hb) atomicAdd(&sh[LS_HBYTES], hb);
        if (!Cap && tid < nd) {
            const u64 x = n.base[ds + tid];
            atomicMin(&sh[LS_MINBASE], x);
            if (x) atomicMax(&sh[LS_MAXBASE], x);
        }
    }
    __syncthreads();
    if constexpr (Cap) {   // a maximum over fractions
        if (tid < 64) {
            const LdPair me = tid < nd ? ld_pair(s.load, tid) : LdPair{0, 1};
            br.fixed = me.l;
            u64 pn = me.l, pd = me.c;
            int pi = tid;
            ld_frac_reduce<true>(pn, pd, pi);
            if (tid == 0) { sh[LS_PEAK0] = pn; sh[LS_PEAK0DEN] = pd; }
        }
    } else if (tid < nd) {
        const u64 x = s.load[tid];
        if (Place) atomicMin(&sh[LS_MINF], x);
        if (x) { atomicMax(&sh[LS_PEAK0], x); atomicAdd(&sh[LS_TOTAL], x); }
    }
    return false;
}

// END, by every lane, t = the tallies of the rounds (zeros without rounds): the peak after, the replicas that left their input dir and
// their bytes, the bound and its proof, the row of per_broker (kLdRow) and the call's counters in ctl.  M = the replicas that may
// change dir, F' = the fixed loads: every replica over base where the residents may move, else the homeless over F.
// The bound without Cap: the maximum of (0) the largest size in M + the smallest F', (1) ceil(sum of L / n), (2) the largest F'.
template <bool Cap, bool X, bool Place>
__device__ __forceinline__ void ld_end(const LdNet &n, LdLds<Cap> &s, const LdBroker &br, const std::conditional_t<X, LdTallyX, LdTally> &t) {
    constexpr LdRow row = kLdRow<Cap, X, Place>;
    const int tid = threadIdx.x, NT = blockDim.x, ds = br.ds, nd = br.nd, nr = br.nr, h = br.h;
    const bool residents = !Place || n.move_residents;
    u64 *sh = s.sh, *o = br.o;
    if (!Cap && tid < nd) {
        const u64 x = s.load[tid];
        if (x) atomicMax(&sh[LS_PEAK1], x);
    }
    if (residents) {
        u64 moved = 0, bytes = 0;
        for (int q = tid; q < nr; q += NT) {
            const int r = br.list[q], d0 = n.dir0[r];
            if (d0 >= 0 && n.dir[r] != d0) { ++moved; bytes += n.size[r]; }   // a placed replica is no move
        }
        if (moved) { atomicAdd(&sh[LS_NMOVED], moved); atomicAdd(&sh[LS_BYTES], bytes); }
        if (t.moves) atomicAdd(&sh[LS_MOVES], t.moves);
        if (t.props) atomicAdd(&sh[LS_PROPS], t.props);
        if constexpr (X) {
            if (t.xch) atomicAdd(&sh[LS_XCH], t.xch);
            if (t.xprops) atomicAdd(&sh[LS_XPROPS], t.xprops);
        }
    }
    __syncthreads();
    const bool any = residents ? nr > 0 : h > 0;   // M is not empty
    int proof = 0;
    if constexpr (Cap) {   // the call's peaks are reduced from the rows on the host
        if (tid >= 64) return;
        const LdPair me = tid < nd ? ld_pair(s.load, tid) : LdPair{0, 1};
        const u64 fixed = !residents ? br.fixed : tid < nd ? n.base[ds + tid] : 0;
        proof = ld_cap_bound(nd, me.l, me.c, fixed, sh[LS_MAXSIZE], any, o + 2);
    }
    if (tid != 0) return;
    if constexpr (Cap) {
        o[0] = sh[LS_PEAK0]; o[1] = sh[LS_PEAK0DEN]; o[row.proof] = (u64)proof;
        if (proof) atomicAdd(&n.ctl[LC_PROVEN], 1ull);
    } else {
        const u64 t0 = any ? sh[LS_MAXSIZE] + (residents ? sh[LS_MINBASE] : sh[LS_MINF]) : 0;
        const u64 t1 = (sh[LS_TOTAL] + sh[LS_HBYTES] + (u64)nd - 1) / (u64)nd;   // sum of F + the homeless = sum of base + every size
        const u64 lb = max(max(t0, t1), residents ? sh[LS_MAXBASE] : sh[LS_PEAK0]);
        o[0] = sh[LS_PEAK0]; o[1] = sh[LS_PEAK1]; o[2] = lb;
        atomicMax(&n.ctl[LC_PEAK0], sh[LS_PEAK0]);
        atomicMax(&n.ctl[LC_PEAK1], sh[LS_PEAK1]);
        if (sh[LS_PEAK1] == lb) atomicAdd(&n.ctl[LC_PROVEN], 1ull);
    }
    o[row.moved] = sh[LS_NMOVED]; o[row.moved + 1] = sh[LS_BYTES]; o[row.moved + 2] = (u64)t.rounds;
    if constexpr (Place) {
        o[row.placed] = (u64)h; o[row.placed + 1] = sh[LS_HBYTES];
        if (h) {
            atomicAdd(&n.ctl[LC_PLACERS], 1ull);
            atomicAdd(&n.ctl[LC_NPLACED], (u64)h);
            atomicAdd(&n.ctl[LC_BPLACED], sh[LS_HBYTES]);
        }
    }
    if constexpr (X) {
        o[row.xch] = (u64)t.xrounds; o[row.xch + 1] = sh[LS_XCH];
        if (t.xrounds) {
            atomicAdd(&n.ctl[LC_XROUNDS], (u64)t.xrounds);
            atomicAdd(&n.ctl[LC_XCH], sh[LS_XCH]);
            atomicAdd(&n.ctl[LC_XPROPS], sh[LS_XPROPS]);
            if (t.xlowered) atomicAdd(&n.ctl[LC_XLOWER], 1ull);
        }
    }
    if (t.rounds) {
        atomicAdd(&n.ctl[LC_BROKERS], 1ull);   // every round with a proposal applies a move
        atomicAdd(&n.ctl[LC_ROUNDS], (u64)t.rounds);
        atomicAdd(&n.ctl[LC_MOVES], sh[LS_MOVES]);
        atomicAdd(&n.ctl[LC_PROPS], sh[LS_PROPS]);
        atomicMax(&n.ctl[LC_MAXROUNDS], (u64)t.rounds);
        atomicAdd(&n.ctl[LC_NMOVED], sh[LS_NMOVED]);
        atomicAdd(&n.ctl[LC_BYTES], sh[LS_BYTES]);
    }
    if (t.more) atomicAdd(&n.ctl[LC_MORE], 1ull);
    if (t.rounds >= kLdHardRounds) atomicAdd(&n.ctl[LC_ERR], 1ull);
}

// ---- kao_balance_logdirs: one broker ---------------------------------------------------------------------------------------------------
// X (kao_balance_logdirs_exchange): dynamic LDS on the LDS path: PI's sizes u64[x_cap], the masks u64[x_mcap], PI's r u32[x_cap]; the
// other path keeps them in xs[], xm[] and sr[] at the bucket's place, which this workgroup alone touches.
template <bool Cap, bool X = false>
__global__ __launch_bounds__(kLdSoloLarge) void k_ld_solve(std::conditional_t<X, LdNetX, LdNet> n) {
    __shared__ LdLds<Cap> s;
    LdBroker br;
    if (ld_begin<Cap, X, false>(n, s, br, [](int, u64) {})) return;
    std::conditional_t<X, LdTallyX, LdTally> t;
    if constexpr (X) {
        extern __shared__ u64 ld_dyn[];
        if (n.x_lds) t = ld_xchg_rounds(n, br, s, ld_dyn, ld_dyn + n.x_cap, reinterpret_cast<uint32_t *>(ld_dyn + n.x_cap + n.x_mcap), n.xp + br.at);
        else t = ld_xchg_rounds(n, br, s, n.xs + br.at, n.xm + br.at + br.ds, n.sr + br.at, n.xp + br.at);
    } else {
        t = ld_rounds<Cap>(n, br, s);
    }
    ld_end<Cap, X, false>(n, s, br, t);
}

// ---- kao_place_logdirs -----------------------------------------------------------------------------------------
// A sort entry is (~size, r): ascending by both is size descending, then r ascending, and the r make every entry distinct.  The
// network is the bitonic one whose comparators all point the same way (the first step of a merge pairs i with i ^ (k - 1), the
// others i with i | j): the lower index takes the lower entry.  The entries from h up to the next power of two are the padding
// that sorts last; no comparator would ever move one, so they are not stored and a comparator that reaches past h is skipped.
template <class K, class I>
__device__ __forceinline__ void ld_sort(K sk, I sr, int h) {
    const int tid = threadIdx.x, NT = blockDim.x;
    int half = 1;
    while (half * 2 < h) half *= 2;   // half the padded length (h >= 2)
    for (int k = 2; k <= 2 * half; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int t = tid; t < half; t += NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // the t-th index with bit j clear
                const int l = j == (k >> 1) ? (i ^ (k - 1)) : (i | j);
                if (l < h) {
                    const u64 ki = sk[i], kl = sk[l];
                    const uint32_t ri = sr[i], rl = sr[l];
                    if (ki > kl || (ki == kl && ri > rl)) { sk[i] = kl; sk[l] = ki; sr[i] = rl; sr[l] = ri; }
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ u64 ld_readlane(u64 x, int lane) {   // lane is the same in every lane
    return (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane) | (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane) << 32;
}

// PLACE by wavefront 0, all 64 lanes active: lane d < nd keeps L(d), the others the maximum.  The sorted entries come in chunks of 64,
// lane j loading entry j; per entry a butterfly over the first `span` lanes (the power of two >= nd) leaves the lowest (L, d) in
// lane 0, a true 64-bit compare with the lane as the tie.  The winner adds the size; lane j keeps the dir of its own entry and
// stores it after the chunk, off the chain.
// Cap: the lowest (L + w) / cap instead, by products; a lane past nd carries the highest key over 1 and sorts after every dir.
// (h, ds and nd come as values, not as the LdBroker: read through the struct, the compiler keeps the bound of the loop over a chunk's
// entries in a vector register and ends every step of the chain with a vector compare.)
template <bool Cap, class K, class I>
__device__ __forceinline__ void ld_greedy(const LdNet &n, LdLds<Cap> &s, K sk, I sr, int h, int ds, int nd) {
    const int lane = threadIdx.x;
    u64 *load = s.load;
    int span = 1;
    while (span < nd) span *= 2;
    u64 L = lane < nd ? ld_load<Cap>(load, lane) : kLdNoKey;
    const u64 C = Cap && lane < nd ? load[2 * lane + 1] : 1;
    for (int c = 0; c < h; c += 64) {
        const int m = min(64, h - c);
        u64 ks = 0;
        uint32_t rr = 0;
        if (lane < m) { ks = sk[c + lane]; rr = sr[c + lane]; }
        int mine = 0;
        for (int i = 0; i < m; ++i) {
            const u64 w = ~ld_readlane(ks, i);
            u64 bl = Cap && lane < nd ? L + w : L;
            int bd = lane;
            if constexpr (Cap) {
                u64 bc = C;
                for (int x = span >> 1; x >= 1; x >>= 1) {
                    const u64 ol = __shfl_xor(bl, x), oc = __shfl_xor(bc, x);
                    const int od = __shfl_xor(bd, x);
                    const u128 theirs = (u128)ol * bc, ours = (u128)bl * oc;
                    const bool lower = theirs < ours || (theirs == ours && od < bd);
                    bl = lower ? ol : bl;
                    bc = lower ? oc : bc;
                    bd = lower ? od : bd;
                }
            } else {
                for (int x = span >> 1; x >= 1; x >>= 1) {
                    const u64 ol = __shfl_xor(bl, x);
                    const int od = __shfl_xor(bd, x);
                    const bool lower = ol < bl || (ol == bl && od < bd);
                    bl = lower ? ol : bl;
                    bd = lower ? od : bd;
                }
            }
            bd = __builtin_amdgcn_readlane(bd, 0);
            if (lane == bd) L += w;
            if (lane == i) mine = bd;
        }
        if (lane < m) n.dir[rr] = ds + mine;
    }
    if (lane < nd) ld_load<Cap>(load, lane) = L;
}

// One workgroup per broker: the loads F of the residents, the homeless replicas compacted and sorted, PLACE, with move_residents the
// rounds over every replica of the broker, then the bound and the row of per_broker.  Dynamic LDS: the sort entries of the LDS path,
// sizes u64[sort_cap] and then r u32[sort_cap]; the other path sorts in key[] and sr[] at the bucket's place, which this workgroup
// alone touches (the rounds write key[] before they read it).
template <bool Cap>
__global__ __launch_bounds__(kLdSoloLarge) void k_ld_place(LdNet n) {
    extern __shared__ u64 ld_dyn[];
    __shared__ LdLds<Cap> s;
    __shared__ int fill;
    const int tid = threadIdx.x;
    u64 *lk = ld_dyn;
    uint32_t *lr = reinterpret_cast<uint32_t *>(ld_dyn + n.sort_cap);
    u64 *gk = n.key + n.start[blockIdx.x];   // the entries of the other path
    uint32_t *sr = n.sr + n.start[blockIdx.x];
    LdBroker br;
    if (tid == 0) fill = 0;   // (the first barrier of BEGIN comes before its pass)
    const bool done = ld_begin<Cap, false, true>(n, s, br, [lk, lr, gk, sr, lds = n.sort_lds](int r, u64 w) {   // a homeless replica into the sort's entries, in any order
        const int e = atomicAdd(&fill, 1);                                       // below h = hcnt[b] <= sort_cap
        if (lds) { lk[e] = ~w; lr[e] = (uint32_t)r; }
        else { gk[e] = ~w; sr[e] = (uint32_t)r; }
    });
    if (done) return;
    const int h = br.h;
    if (h >= 2) {
        if (n.sort_lds) ld_sort(lk, lr, h);
        else ld_sort(gk, sr, h);
    }
    if (h >= 1) {
        if (tid < 64) {
            if (n.sort_lds) ld_greedy<Cap>(n, s, lk, lr, h, br.ds, br.nd);
            else ld_greedy<Cap>(n, s, gk, sr, h, br.ds, br.nd);
        }
        __syncthreads();   // the loads and the dirs of the placed replicas, for every lane
    }
    LdTally t;
    if (n.move_residents) t = ld_rounds<Cap>(n, br, s);
    ld_end<Cap, false, true>(n, s, br, t);
}

thread_local int t_ld_sort = 0;   // kao_logdirs_test_sort: 0 = by size, 1 = dynamic LDS, 2 = global memory
thread_local int t_ld_xchg = 0;   // kao_logdirs_test_exchange: the same three for PI and the masks of kao_balance_logdirs_exchange

int validate_logdirs(const std::string &fn, int32_t B, const int32_t *dir_start, const uint64_t *base, int32_t R, const int32_t *dir, const uint64_t *size,
                     const void *const *outs, int n_outs, int lowest_dir = 0) {
    bool null = !dir_start || !dir || !size;
    for (int i = 0; i < n_outs; ++i) null |= !outs[i];
    if (null) return fail(KAO_ERR_INVALID, fn + "null pointer");
    if (B < 1 || B > 65534) return fail(KAO_ERR_INVALID, fn + "n_brokers must be 1..65534");
    if (dir_start[0] != 0) return fail(KAO_ERR_INVALID, fn + "dir_start[0] must be 0");
    for (int b = 0; b < B; ++b)
        if (dir_start[b + 1] < dir_start[b]) return fail(KAO_ERR_INVALID, fn + "dir_start decreases at broker " + std::to_string(b));
    if (R < 0) return fail(KAO_ERR_INVALID, fn + "n_replicas must be >= 0");
    for (int b = 0; b < B; ++b)
        if (dir_start[b + 1] - dir_start[b] > kLdMaxDirs)
            return fail(KAO_ERR_UNSUPPORTED, fn + "broker " + std::to_string(b) + " has more than " + std::to_string(kLdMaxDirs) + " dirs (a wavefront ranks the dirs of a broker)");
    if (R > kLdMaxReplicas) return fail(KAO_ERR_UNSUPPORTED, fn + "more than 4,000,000 replicas");
    const int32_t D = dir_start[B];
    for (int64_t r = 0; r < R; ++r)
        if (dir[r] < lowest_dir || dir[r] >= D)
            return fail(KAO_ERR_INVALID, fn + "dir[" + std::to_string(r) + "] is outside " + (lowest_dir ? "-1" : "0") + "..n_dirs-1");
    uint64_t total = 0;   // below 2^62: every load of the kernel stays below 2^63
    const uint64_t lim = uint64_t(1) << 62;
    for (int64_t d = 0; base && d < D; ++d)
        if (__builtin_add_overflow(total, base[d], &total) || total >= lim) return fail(KAO_ERR_INVALID, fn + "base and size sum to 2^62 or more");
    for (int64_t r = 0; r < R; ++r)
        if (__builtin_add_overflow(total, size[r], &total) || total >= lim) return fail(KAO_ERR_INVALID, fn + "base and size sum to 2^62 or more");
    return KAO_OK;
}

// the capacity calls: every cap[d] >= 1 and a sum below 2^62, so with the loads below 2^62 every product of the two fits 128 bits
int validate_capacity(const std::string &fn, int32_t D, const uint64_t *cap) {
    uint64_t total = 0;
    for (int64_t d = 0; d < D; ++d) {
        if (cap[d] == 0) return fail(KAO_ERR_INVALID, fn + "cap[" + std::to_string(d) + "] is 0");
        if (__builtin_add_overflow(total, cap[d], &total) || total >= (uint64_t(1) << 62)) return fail(KAO_ERR_INVALID, fn + "the capacities sum to 2^62 or more");
    }
    return KAO_OK;
}

// {L, cap} of the fullest dir of the call from the rows of per_broker (W columns, the fraction at column `at`): the brokers in
// order, a later one only when strictly fuller, so ties go to the lowest dir index; {0, 1} without dirs
void peak_of_rows(const int32_t *dir_start, int B, const uint64_t *per_broker, int W, int at, uint64_t out[2]) {
    bool have = false;
    out[0] = 0; out[1] = 1;
    for (int b = 0; b < B; ++b) {
        if (dir_start[b + 1] == dir_start[b]) continue;
        const uint64_t *o = per_broker + (size_t)W * b + at;
        if (!have || (u128)o[0] * out[1] > (u128)out[0] * o[1]) { out[0] = o[0]; out[1] = o[1]; have = true; }
    }
}

// ---- one call on the host, from checked arguments to filled outputs ---------------------------------------------------------------------
// open: the arena, the uploads, the buckets by broker (keyed by broker[r], or without broker[] by the broker of dir[r]), the lanes of
// a broker's workgroup and the kernel arguments that every call has.  The caller then chooses its path, completes n and launches its
// kernel; finish: the read-back and the outputs that every call has.  cap, broker and x say which optional buffers the arena holds:
//   ctl u64[LC_N] | cnt i32[B] | broker: hcnt i32[B] | base u64[D] (zeroed up to here) | start, fill i32[B] | dir_start i32[B + 1] |
//   broker i32[R], else the broker of every dir i32[D] | per_broker u64[W * B] | key, size u64[R] | dir, dir0, list i32[R] | dst u8[R] |
//   broker or x: sr u32[R] | cap u64[D] | x: xs u64[R] | xm u64[R + D] | xp u32[R]
struct LdCall {
    CallBufs m;
    LdNetX n{};                 // k_ld_solve<Cap> and k_ld_place take the LdNet of it
    const int32_t *dir_start = nullptr;
    int B = 0, R = 0, W = 0, launches = 0, threads = 0;
    u64 max_n[2] = {0, 0};      // the largest bucket, the most homeless replicas of one broker
    u64 ctl[LC_N];              // after finish

    int open(int32_t n_brokers, const int32_t *dir_start_, const uint64_t *base, const uint64_t *cap, int32_t n_replicas, const int32_t *broker,
             const int32_t *dir, const uint64_t *size, uint64_t min_gain, int32_t max_rounds, int row_width, bool x) {
        dir_start = dir_start_; B = n_brokers; R = n_replicas; W = row_width;
        const int D = dir_start[B];
        std::vector<int32_t> bod;   // broker_of_dir
        if (!broker) {
            bod.assign((size_t)std::max(D, 1), 0);
            for (int b = 0; b < B; ++b)
                for (int d = dir_start[b]; d < dir_start[b + 1]; ++d) bod[(size_t)d] = b;
        }
        Carve cv;
        const size_t o_ctl = cv.take<u64>(LC_N), o_cnt = cv.take<int32_t>(B), o_hcnt = cv.take<int32_t>(broker ? B : 0), o_base = cv.take<u64>(D), zeroed = cv.end(),
                     o_start = cv.take<int32_t>(B), o_fill = cv.take<int32_t>(B), o_ds = cv.take<int32_t>((size_t)B + 1), o_idx = cv.take<int32_t>(broker ? R : D),
                     o_pb = cv.take<u64>(W * (size_t)B), o_key = cv.take<u64>(R), o_size = cv.take<u64>(R), o_dir = cv.take<int32_t>(R), o_dir0 = cv.take<int32_t>(R),
                     o_list = cv.take<int32_t>(R), o_dst = cv.take<uint8_t>(R), o_sr = cv.take<uint32_t>(broker || x ? R : 0), o_cap = cv.take<u64>(cap ? D : 0),
                     o_xs = cv.take<u64>(x ? R : 0), o_xm = cv.take<u64>(x ? (size_t)R + D : 0), o_xp = cv.take<uint32_t>(x ? R : 0);
        int rc = m.open(cv.end());
        if (rc) return rc;
        hipStream_t st = m.stream;
        int32_t *d_cnt = m.at<int32_t>(o_cnt), *d_hcnt = broker ? m.at<int32_t>(o_hcnt) : nullptr, *d_start = m.at<int32_t>(o_start), *d_fill = m.at<int32_t>(o_fill),
                *d_ds = m.at<int32_t>(o_ds), *d_idx = m.at<int32_t>(o_idx), *d_dir = m.at<int32_t>(o_dir), *d_dir0 = m.at<int32_t>(o_dir0), *d_list = m.at<int32_t>(o_list);
        u64 *d_ctl = m.at<u64>(o_ctl), *d_base = m.at<u64>(o_base), *d_size = m.at<u64>(o_size), *d_cap = cap ? m.at<u64>(o_cap) : nullptr;

        HIP_TRY(hipMemsetAsync(m.arena, 0, zeroed, st));
        HIP_TRY(hipMemcpyAsync(d_ds, dir_start, ((size_t)B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (D) {
            if (!broker) HIP_TRY(hipMemcpyAsync(d_idx, bod.data(), (size_t)D * sizeof(int32_t), hipMemcpyHostToDevice, st));
            if (base) HIP_TRY(hipMemcpyAsync(d_base, base, (size_t)D * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            if (cap) HIP_TRY(hipMemcpyAsync(d_cap, cap, (size_t)D * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        }
        if (R) {
            if (broker) HIP_TRY(hipMemcpyAsync(d_idx, broker, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_dir0, dir, (size_t)R * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_dir, d_dir0, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_size, size, (size_t)R * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        }
        const int32_t *key_of = broker ? d_idx : d_dir0, *map = broker ? nullptr : d_idx;   // the broker of r is map[key_of[r]], key_of[r] without a map
        const unsigned rblocks = grid_for(R, kLdThreads);
        if (R) {
            k_ld_count<<<rblocks, kLdThreads, 0, st>>>(R, key_of, map, d_dir0, d_cnt, d_hcnt);
            ++launches;
        }
        k_bucket_offsets<<<1, 1024, 0, st>>>(B, d_cnt, d_hcnt, d_start, d_fill, d_ctl + LC_MAXN);
        ++launches;
        if (R) {
            k_ld_scatter<<<rblocks, kLdThreads, 0, st>>>(R, key_of, map, d_start, d_fill, d_list);
            ++launches;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(max_n, d_ctl + LC_MAXN, sizeof max_n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        threads = max_n[0] <= (u64)kLdSmallBucket ? kLdSoloSmall : kLdSoloLarge;

        n.max_rounds = max_rounds; n.min_gain = min_gain; n.dir_start = d_ds; n.base = d_base; n.size = d_size; n.dir = d_dir; n.dir0 = d_dir0;
        n.cnt = d_cnt; n.start = d_start; n.list = d_list; n.key = m.at<u64>(o_key); n.dst = m.at<uint8_t>(o_dst); n.per_broker = m.at<u64>(o_pb); n.ctl = d_ctl;
        n.move_residents = 1; n.hcnt = d_hcnt; n.sr = broker || x ? m.at<uint32_t>(o_sr) : nullptr; n.cap = d_cap;
        if (x) { n.xs = m.at<u64>(o_xs); n.xm = m.at<u64>(o_xm); n.xp = m.at<uint32_t>(o_xp); }
        return KAO_OK;
    }

    // after the caller's launch; peak_before and peak_after are fractions {L, cap} in a capacity call
    int finish(const std::string &fn, int32_t *dir, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
               uint64_t *per_broker, int32_t *status) {
        hipStream_t st = m.stream;
        HIP_TRY(hipGetLastError());
        ++launches;
        HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(per_broker, n.per_broker, (size_t)B * W * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ctl[LC_ERR]) return fail(KAO_ERR_HIP, fn + "the rounds did not finish");
        if (!dry_run && (ctl[LC_NPLACED] || ctl[LC_NMOVED])) {
            HIP_TRY(hipMemcpyAsync(dir, n.dir, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        *n_moved = (int32_t)ctl[LC_NMOVED];
        *bytes_moved = ctl[LC_BYTES];
        if (n.cap) {
            peak_of_rows(dir_start, B, per_broker, W, 0, peak_before);
            peak_of_rows(dir_start, B, per_broker, W, 2, peak_after);
        } else {
            *peak_before = ctl[LC_PEAK0];
            *peak_after = ctl[LC_PEAK1];
        }
        *status = ctl[LC_PROVEN] == (u64)B ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
        return KAO_OK;
    }
};

// the entry points: Cap (cap != NULL) is the descent by utilisation: the other instantiation of the kernels, rows of 10 / 12 columns
// with fractions, the call's peaks reduced from the rows
// X (kao_balance_logdirs_exchange): k_ld_solve<false, true>, rows of 8 columns, stats[12]
template <bool Cap, bool X = false>
int balance_logdirs(const std::string &fn, int32_t n_brokers, const int32_t *dir_start, const uint64_t *base, const uint64_t *cap, int32_t n_replicas,
                    int32_t *dir, const uint64_t *size, uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                    uint64_t *peak_before, uint64_t *peak_after, uint64_t *per_broker, int32_t *status, int64_t *stats) {
    const void *outs[] = {n_moved, bytes_moved, peak_before, peak_after, per_broker, status, Cap ? (const void *)cap : (const void *)status};
    int rc = validate_logdirs(fn, n_brokers, dir_start, base, n_replicas, dir, size, outs, 7);
    if (rc) return rc;
    if (Cap && (rc = validate_capacity(fn, dir_start[n_brokers], cap))) return rc;
    if ((rc = require_init())) return rc;
    LdCall c;
    if ((rc = c.open(n_brokers, dir_start, base, cap, n_replicas, nullptr, dir, size, min_gain, max_rounds, kLdRow<Cap, X, false>.w, X))) return rc;
    if constexpr (X) {   // PI and the masks in LDS when those of the largest bucket, with the most dirs of a broker, fit
        const u64 max_n = c.max_n[0];
        int max_nd = 0;
        for (int b = 0; b < n_brokers; ++b) max_nd = std::max(max_nd, dir_start[b + 1] - dir_start[b]);
        const size_t mcap = (size_t)max_nd * (size_t)(max_n / 64 + 1);
        const size_t bytes = (size_t)max_n * (sizeof(u64) + sizeof(uint32_t)) + mcap * sizeof(u64);
        const bool fits = max_n <= (u64)kLdSortLds && bytes <= (size_t)kLdXchgLds;   // the sort's limit of k_ld_place, and the masks beside the entries
        if (t_ld_xchg == 1 && !fits)
            return fail(KAO_ERR_UNSUPPORTED, fn + "a broker's " + std::to_string(max_n) + " replicas on " + std::to_string(max_nd) + " dirs need " +
                                                 std::to_string(bytes) + " bytes of LDS: more than the " + std::to_string(kLdXchgLds) + " of the LDS path");
        const bool lds = t_ld_xchg == 2 ? false : fits;
        c.n.x_lds = lds ? 1 : 0; c.n.x_cap = lds ? (int)max_n : 0; c.n.x_mcap = lds ? (int)mcap : 0;
        k_ld_solve<false, true><<<(unsigned)n_brokers, c.threads, lds ? bytes : 0, c.m.stream>>>(c.n);
    } else {
        k_ld_solve<Cap><<<(unsigned)n_brokers, c.threads, 0, c.m.stream>>>(c.n);
    }
    if ((rc = c.finish(fn, dir, dry_run, n_moved, bytes_moved, peak_before, peak_after, per_broker, status))) return rc;
    const u64 *ctl = c.ctl;
    if (stats) {
        stats[0] = (int64_t)ctl[LC_BROKERS]; stats[1] = (int64_t)ctl[LC_ROUNDS]; stats[2] = (int64_t)ctl[LC_MOVES]; stats[3] = (int64_t)ctl[LC_PROPS];
        stats[4] = c.launches; stats[5] = (int64_t)ctl[LC_MORE]; stats[6] = (int64_t)ctl[LC_PROVEN]; stats[7] = (int64_t)ctl[LC_MAXROUNDS];
        if (X) { stats[8] = (int64_t)ctl[LC_XROUNDS]; stats[9] = (int64_t)ctl[LC_XCH]; stats[10] = (int64_t)ctl[LC_XPROPS]; stats[11] = (int64_t)ctl[LC_XLOWER]; }
    }
    return KAO_OK;
}

template <bool Cap>
int place_logdirs(const std::string &fn, int32_t n_brokers, const int32_t *dir_start, const uint64_t *base, const uint64_t *cap, int32_t n_replicas,
                  const int32_t *broker, int32_t *dir, const uint64_t *size, int32_t move_residents, uint64_t min_gain, int32_t max_rounds, int32_t dry_run,
                  int32_t *n_placed, uint64_t *bytes_placed, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
                  uint64_t *per_broker, int32_t *status, int64_t *stats) {
    const void *outs[] = {broker, n_placed, bytes_placed, n_moved, bytes_moved, peak_before, peak_after, per_broker, status, Cap ? (const void *)cap : (const void *)status};
    int rc = validate_logdirs(fn, n_brokers, dir_start, base, n_replicas, dir, size, outs, 10, -1);
    if (rc) return rc;
    const int B = n_brokers, R = n_replicas, D = dir_start[B];
    for (int64_t r = 0; r < R; ++r) {
        const int32_t b = broker[r], d = dir[r];
        if (b < 0 || b >= B) return fail(KAO_ERR_INVALID, fn + "broker[" + std::to_string(r) + "] is outside 0..n_brokers-1");
        if (d >= 0 && (d < dir_start[b] || d >= dir_start[b + 1]))
            return fail(KAO_ERR_INVALID, fn + "dir[" + std::to_string(r) + "] is not a dir of broker " + std::to_string(b));
        if (d < 0 && dir_start[b + 1] == dir_start[b])
            return fail(KAO_ERR_INVALID, fn + "replica " + std::to_string(r) + " is homeless on broker " + std::to_string(b) + ", which has no dir");
    }
    if (Cap && (rc = validate_capacity(fn, D, cap))) return rc;
    if ((rc = require_init())) return rc;
    LdCall c;
    if ((rc = c.open(B, dir_start, base, cap, R, broker, dir, size, min_gain, max_rounds, kLdRow<Cap, false, true>.w, false))) return rc;
    const u64 max_h = c.max_n[1];
    const bool fits = max_h <= (u64)kLdSortLds;
    if (t_ld_sort == 1 && !fits)
        return fail(KAO_ERR_UNSUPPORTED, fn + "a broker has " + std::to_string(max_h) + " homeless replicas: more than the " + std::to_string(kLdSortLds) +
                                             " the LDS sort holds");
    const bool lds = t_ld_sort == 2 ? false : fits;
    c.n.move_residents = move_residents ? 1 : 0; c.n.sort_lds = lds ? 1 : 0; c.n.sort_cap = lds ? (int)max_h : 0;
    k_ld_place<Cap><<<(unsigned)B, c.threads, (size_t)c.n.sort_cap * (sizeof(u64) + sizeof(uint32_t)), c.m.stream>>>(c.n);
    if ((rc = c.finish(fn, dir, dry_run, n_moved, bytes_moved, peak_before, peak_after, per_broker, status))) return rc;
    const u64 *ctl = c.ctl;
    *n_placed = (int32_t)ctl[LC_NPLACED];
    *bytes_placed = ctl[LC_BPLACED];
    if (stats) {
        stats[0] = (int64_t)ctl[LC_PLACERS]; stats[1] = (int64_t)ctl[LC_BROKERS]; stats[2] = (int64_t)ctl[LC_ROUNDS]; stats[3] = (int64_t)ctl[LC_MOVES];
        stats[4] = (int64_t)ctl[LC_PROPS]; stats[5] = c.launches; stats[6] = (int64_t)ctl[LC_MORE]; stats[7] = (int64_t)ctl[LC_PROVEN];
        stats[8] = (int64_t)ctl[LC_MAXROUNDS]; stats[9] = (int64_t)max_h;
    }
    return KAO_OK;
}

}  // namespace

extern "C" int kao_balance_logdirs(int32_t n_brokers, const int32_t *dir_start, const uint64_t *base, int32_t n_replicas, int32_t *dir, const uint64_t *size,
                                   uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before,
                                   uint64_t *peak_after, uint64_t *per_broker, int32_t *status, int64_t stats[8]) {
    return balance_logdirs<false>("kao_balance_logdirs: ", n_brokers, dir_start, base, nullptr, n_replicas, dir, size, min_gain, max_rounds, dry_run, n_moved,
                                  bytes_moved, peak_before, peak_after, per_broker, status, stats);
}

extern "C" int kao_balance_logdirs_capacity(int32_t n_brokers, const int32_t *dir_start, const uint64_t *base, const uint64_t *cap, int32_t n_replicas,
                                            int32_t *dir, const uint64_t *size, uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_moved,
                                            uint64_t *bytes_moved, uint64_t peak_before[2], uint64_t peak_after[2], uint64_t *per_broker, int32_t *status,
                                            int64_t stats[8]) {
    return balance_logdirs<true>("kao_balance_logdirs_capacity: ", n_brokers, dir_start, base, cap, n_replicas, dir, size, min_gain, max_rounds, dry_run, n_moved,
                                 bytes_moved, peak_before, peak_after, per_broker, status, stats);
}

extern "C" int kao_balance_logdirs_exchange(int32_t n_brokers, const int32_t *dir_start, const uint64_t *base, int32_t n_replicas, int32_t *dir,
                                            const uint64_t *size, uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                                            uint64_t *peak_before, uint64_t *peak_after, uint64_t *per_broker, int32_t *status, int64_t stats[12]) {
    return balance_logdirs<false, true>("kao_balance_logdirs_exchange: ", n_brokers, dir_start, base, nullptr, n_replicas, dir, size, min_gain, max_rounds, dry_run,
                                        n_moved, bytes_moved, peak_before, peak_after, per_broker, status, stats);
}

extern "C" int kao_logdirs_test_exchange(int32_t path) {
    if (path < 0 || path > 2) return fail(KAO_ERR_INVALID, "kao_logdirs_test_exchange: path outside 0..2");
    const int was = t_ld_xchg;
    t_ld_xchg = path;
    return was;
}

extern "C" int kao_logdirs_test_sort(int32_t path) {
    if (path < 0 || path > 2) return fail(KAO_ERR_INVALID, "kao_logdirs_test_sort: path outside 0..2");
    const int was = t_ld_sort;
    t_ld_sort = path;
    return was;
}

extern "C" int kao_place_logdirs(int32_t n_brokers, const int32_t *dir_start, const uint64_t *base, int32_t n_replicas, const int32_t *broker, int32_t *dir,
                                 const uint64_t *size, int32_t move_residents, uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_placed,
                                 uint64_t *bytes_placed, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
                                 uint64_t *per_broker, int32_t *status, int64_t stats[10]) {
    return place_logdirs<false>("kao_place_logdirs: ", n_brokers, dir_start, base, nullptr, n_replicas, broker, dir, size, move_residents, min_gain, max_rounds,
                                dry_run, n_placed, bytes_placed, n_moved, bytes_moved, peak_before, peak_after, per_broker, status, stats);
}

extern "C" int kao_place_logdirs_capacity(int32_t n_brokers, const int32_t *dir_start, const uint64_t *base, const uint64_t *cap, int32_t n_replicas,
                                          const int32_t *broker, int32_t *dir, const uint64_t *size, int32_t move_residents, uint64_t min_gain,
                                          int32_t max_rounds, int32_t dry_run, int32_t *n_placed, uint64_t *bytes_placed, int32_t *n_moved, uint64_t *bytes_moved,
                                          uint64_t peak_before[2], uint64_t peak_after[2], uint64_t *per_broker, int32_t *status, int64_t stats[10]) {
    return place_logdirs<true>("kao_place_logdirs_capacity: ", n_brokers, dir_start, base, cap, n_replicas, broker, dir, size, move_residents, min_gain,
                               max_rounds, dry_run, n_placed, bytes_placed, n_moved, bytes_moved, peak_before, peak_after, per_broker, status, stats);
}
