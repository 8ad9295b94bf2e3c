// kao_disk.hip -- kao_balance_disk: replica moves that lower the peak of the bytes a broker stores, S(b) = sum of size[p] over the
// rows that contain b, and kao_balance_disk_budget: the same under a budget of bytes copied (section 4n);
// kao_balance_disk_capacity (section 4q) and kao_balance_disk_exchange (section 4u; its text stands before its kernels below).
// Kernels and the C entry points.
//
// A move takes the replica in slot j of row p from broker a to a broker c OUTSIDE the row; the slot keeps its place.  c is
// admissible iff it is not in the row and (no rack rule, or rack(c) == rack(a), or the row holds fewer than max_per_rack brokers of
// rack(c)).  Slot 0 moves only with move_leaders.  Minimising the peak is makespan scheduling (NP-hard), so this is the deterministic
// parallel DESCENT of section 4k with another move, and a lower bound beside it.  A ROUND uses the loads as they stand at its start:
//   1. RANK the brokers by S descending (ties: index ascending); order[r] = the broker of rank r;
//   2. every partition with size > 0 takes its movable slots heaviest broker first; for slot j on a of rank r, c1 = the first
//      admissible broker among the ranks B-1-r, B-2-r, .., r+1 (the i-th heaviest is paired with the i-th lightest, then the walk goes
//      toward the heavier); it PROPOSES (p, j, a -> c1) iff S(c1) + size + min_gain < S(a); otherwise c2 = the first admissible among
//      the ranks B-1, B-2, .., B-r (the lighter ones the first walk skipped) under the same test; otherwise the next slot.  A walk
//      stops at its first admissible broker: every later one is heavier;
//   3. key = rank(a) << 48 | (0xFFFF - code(size[p])) << 32 | p, code = wave_bytes_code: the heaviest source (exact), then the heaviest
//      partition, then the lowest index;
//   4. a proposal WINS iff its key is the lowest of all proposals that touch a and of all that touch c: one descent_bid per
//      participant into minkey[b].  Winners share no broker and no partition wins twice, so row[j] = c, S(a) -= size, S(c) += size
//      are plain stores;
//   5. until a round has no proposal (or max_rounds rounds have run).
// The globally lowest key wins at both its brokers, every move lowers sum S^2 by 2w(S(a) - S(c) - w) > 0 and leaves both loads below
// the old S(a): the rounds end and the peak never rises.
// The snapshot "loads as of the round's start" holds by construction: a round is three kernels that do not overlap.  RANK reads the
// loads and writes rank[] and order[]; PROPOSE reads loads, ranks and rows and writes key[p], slot[p], dest[p] and the round's minkey
// row; APPLY reads what its lane owns and the minkey row, and the winners write rows and loads.  Two minkey rows rotate (the apply of
// round r clears the row of round r + 1); the host reads the rounds' proposal counts every kDkBatch rounds, and the rounds enqueued
// after the first empty one change nothing (no proposal, no winner, the same ranks).
// The lower bound holds for every state the moves can reach: max(max size, ceil(sum k_p size[p] / B), and, when the leaders stay,
// the largest sum of the slot-0 replicas of one broker).  Integers only.
//
// UNDER A BUDGET (kao_balance_disk_budget) a move (p, j, a -> c) COSTS size[p] * ([c not in in(p)] - [a not in in(p)]), in(p) = the
// input row: +size, 0, or -size when a fresh copy goes home, so the costs of the applied moves sum to bytes_moved.  Its CHARGE is
// max(cost, 0), and rem = max_bytes - spent at the round's start.  PROPOSE<true> takes c as a candidate only if charge <= rem; a new
// kernel GRANT, between propose and apply, settles the winners from the broker side: in rank order q, order[q] is the source of a
// winner iff its minkey word carries rank q and the destination's word holds the same key; a winner with a charge is granted iff the
// charges of all winners of lower source rank plus its own are <= rem (one workgroup, a block scan over the ranks).  APPLY<true>
// applies the granted winners and adds their costs to spent (one wrapping u64 add per wavefront).  The lowest key of a round has
// the lowest source rank, so its prefix is its own charge <= rem: every round with a proposal still applies a move.
//
// BY UTILISATION (kao_balance_disk_capacity, section 4q) broker b has cap[b] bytes of disk and the peak to lower is that of
// u(b) = S(b) / cap(b), never computed as a quotient: x / cx is above y / cy iff x * cy > y * cx in 128 bits.  RANK<Cap> ranks by u; the
// gain test is (S(c) + size + min_gain) * cap(a) < S(a) * cap(c); and "every later one is heavier" no longer means "every later one
// fails", so once a FAST round (the two walks above) has no proposal every later round is THOROUGH: one walk over the ranks
// B-1 .. r+1 that takes the first admissible, affordable broker that PASSES the test.  A broker that passes is strictly emptier than
// a, so it ranks behind a: the THOROUGH walk sees every move there is, and a round of it without a proposal ends the descent.  A
// winner leaves both of its brokers strictly below the old u(a), so the utilisations sorted descending fall lexicographically.
// Grant, apply and finish work on ranks and bytes and are the ones above.
//
// DRAINING (kao_balance_disk_drain, section 4w) D of the brokers are to end empty.  RANK puts them before every live broker (inside
// each group S descending, then index ascending), so "broker x is draining" is "rank(x) < D" everywhere below and costs no load of
// its own: a walk never goes below rank D (nothing moves onto a draining broker), a slot whose broker ranks below D is always movable
// (slot 0 and size 0 included), and its proposal takes c1, else c2, without a gain test.  Key, bid, win and apply are the ones above:
// the rank in the key puts the drain moves first, and a draining broker gives up one replica a round.  The peak may rise meanwhile.
//
// INSIDE A COUNT BAND (kao_balance_disk_banded, section 4x) n(b) = the rows that contain b (size 0 included), taken like the loads as it
// stands at the round's start.  A destination must also have n(c) < count_hi and a slot on a is movable only with n(a) > count_lo.
// Winners share no broker, so a count changes by at most one a round: the test on the round's start is never overshot and the winners
// update n with plain stores.  RANK writes one 16-bit word per broker, rack | full << 8 | floor << 9, which the walks read IN PLACE of
// rack[c]: a candidate costs what it cost.  The exchange rounds keep every count and are the ones below, untouched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "kao_host.h"
#include "kao_plan_dev.h"   // descent_gains, descent_bid, lane_count_to, wave_max_to, wave_sum_to, rank_ahead, wave_bytes_code

namespace {

constexpr int kDkThreads = 256;
constexpr int kDkBatch = 32;            // rounds enqueued between two reads of the proposal counts
constexpr int kDkThoroughBatch = 4;     // ... of THOROUGH rounds: few of them have a proposal, and an empty one costs a full walk per slot
constexpr int kDkHardRounds = 1 << 26;  // no descent gets here; a guard against an endless loop
constexpr u64 kDkNoKey = ~0ull;
constexpr int kDkGrantThreads = 1024;   // k_dk_grant: one workgroup, one rank per lane and chunk
enum { D_PEAK0 = 0, D_PEAK1, D_MOVES, D_MAXSIZE, D_TOTAL, D_FIXED, D_NMOVED, D_BYTES, D_ROWS, D_BROKERS, D_SPENT, D_REFUSED, D_XCH, D_XPEAK, D_XSEEN, D_DONE, D_DRAINED, D_LASTDRAIN, D_NLEFT, D_BLEFT, D_CMIN0, D_CMAX0, D_CMIN1, D_CMAX1, D_OUT0, D_OUT1, D_N = 26 };
constexpr int kDkFull = 0x100, kDkFloor = 0x200;   // the band's word of a broker: n(b) >= count_hi, n(b) <= count_lo; the rack below them
constexpr u64 kDkCountTop = 0x7FFFFFFF;             // a minimum of counts travels as the maximum of kDkCountTop - n (ctl starts at 0)

struct DkNet {   // one call; every pointer is device memory
    int P, W, B, cap, first;   // first = the lowest movable slot: 0 with move_leaders, else 1
    u64 min_gain;
    uint16_t *rows;            // [PW] rewritten by the winners
    const uint16_t *rows0;     // [PW] the input
    const u64 *size;           // [P]
    const uint8_t *rack;       // [B]
    uint8_t *slot;             // [P] slot proposed in this round
    uint16_t *dest;            // [P] its destination
    u64 *key;                  // [P] key of this round's proposal, kDkNoKey = none
    u64 *load;                 // [B]
    int32_t *rank, *order;     // [B] rank of a broker, broker of a rank
    u64 *mk;                   // [2][B] minkey rows
    u64 *ctl;                  // [D_N]
    uint8_t *grant;            // [B] under a budget: the winner that leaves b is applied in this round
    u64 max_bytes;             // the budget; ctl[D_SPENT] = the costs of the moves applied so far
    const u64 *capacity;       // [B] by utilisation only: the bytes of disk a broker has
    int nd;                    // draining only: D, the number of draining brokers (they hold the ranks 0 .. D-1); 0 in every other call
    const uint8_t *drain;      // [B] draining only: != 0 for a broker that is to end empty
};

// inside a count band: the net of the call (DkNet, or DkNetX with exchanges) and the band's own words behind it, so that the kernels of
// the other calls keep their arguments
template <class Base>
struct DkBandNet : Base {
    int32_t *cnt;              // [B] n(b), kept current by the winners of the move rounds
    uint16_t *rf;              // [B] rack | kDkFull | kDkFloor as of the round's start, written by k_dk_rank_band
    int32_t lo, hi;            // the band
};

// ---- once per call ------------------------------------------------------------------------------------------------------------------
// loads, the largest size, sum k_p size[p], the bytes of the slot-0 replicas per broker (Drain: per LIVE broker; a draining one's leave)
// (Band: and the counts, one atomic add per replica, size 0 included)
template <bool Drain, bool Band, class Net>
__device__ __forceinline__ void dk_init(const Net n, u64 *fixed) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    u64 w = 0, all = 0;
    if (p < n.P) {
        w = n.size[p];
        n.key[p] = kDkNoKey;
        const uint16_t *row = n.rows0 + (size_t)p * n.W;
        if constexpr (Band) {
            for (int j = 0; j < n.W && row[j] != KAO_NONE; ++j) atomicAdd(&n.cnt[row[j]], 1);
        }
        if (w) {
            for (int j = 0; j < n.W; ++j) {
                const int x = row[j];
                if (x == KAO_NONE) break;
                atomicAdd(&n.load[x], w);
                all += w;
            }
            if (!Drain || n.drain[row[0]] == 0) atomicAdd(&fixed[row[0]], w);
        }
    }
    wave_max_to(w, &n.ctl[D_MAXSIZE]);
    wave_sum_to(all, &n.ctl[D_TOTAL]);
}

template <bool Drain>
__global__ void k_dk_init(DkNet n, u64 *__restrict__ fixed) { dk_init<Drain, false>(n, fixed); }
__global__ void k_dk_init_band(DkBandNet<DkNet> n, u64 *__restrict__ fixed) { dk_init<false, true>(n, fixed); }

// inside a band, beside either peak: the lowest and the highest count and the brokers outside the band, into ctl[at .. at + 1] and ctl[out]
__device__ __forceinline__ void dk_count_range(const DkBandNet<DkNet> &n, int b, int at, int out) {
    const int c = b < n.B ? n.cnt[b] : 0;
    wave_max_to(b < n.B ? kDkCountTop - (u64)c : 0, &n.ctl[at]);
    wave_max_to((u64)c, &n.ctl[at + 1]);
    lane_count_to(b < n.B && (c < n.lo || c > n.hi), &n.ctl[out]);
}

// the peak before and the largest fixed load; the loads kept for the finish
__device__ __forceinline__ void dk_peak0(const DkNet &n, const u64 *fixed, u64 *load0) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    u64 s = 0, f = 0;
    if (b < n.B) {
        s = n.load[b];
        f = fixed[b];
        load0[b] = s;
    }
    wave_max_to(s, &n.ctl[D_PEAK0]);
    wave_max_to(f, &n.ctl[D_FIXED]);
}

__global__ void k_dk_peak0(DkNet n, const u64 *__restrict__ fixed, u64 *__restrict__ load0) { dk_peak0(n, fixed, load0); }
__global__ void k_dk_peak0_band(DkBandNet<DkNet> n, const u64 *__restrict__ fixed, u64 *__restrict__ load0) {
    dk_peak0(n, fixed, load0);
    dk_count_range(n, blockIdx.x * blockDim.x + threadIdx.x, D_CMIN0, D_OUT0);
}

// ---- a round ------------------------------------------------------------------------------------------------------------------------
// rank[b] = brokers ahead of b by (load descending, index ascending), order[rank[b]] = b.  Cap: by utilisation, x ahead of b iff
// load(x) * cap(b) > load(b) * cap(x), or the products are equal and x < b (rank_ahead of kao_plan_dev.h)
template <bool Cap>
__global__ __launch_bounds__(kDkThreads) void k_dk_rank(int B, const u64 *__restrict__ load, const u64 *__restrict__ capacity, int32_t *__restrict__ rank,
                                                        int32_t *__restrict__ order) {
    const int b = blockIdx.x * kDkThreads + threadIdx.x;
    const u64 mine = b < B ? load[b] : 0, mcap = Cap && b < B ? capacity[b] : 1;
    const int r = rank_ahead<kDkThreads, Cap>(B, b, mine, mcap, load, capacity);
    if (b < B) {   // ranks are a permutation: r < B
        rank[b] = r;
        order[r] = b;
    }
}

// ... with draining brokers: they rank before every live one (rank_ahead with a first group)
__global__ __launch_bounds__(kDkThreads) void k_dk_rank_drain(int B, const u64 *__restrict__ load, const uint8_t *__restrict__ drain, int32_t *__restrict__ rank,
                                                              int32_t *__restrict__ order) {
    const int b = blockIdx.x * kDkThreads + threadIdx.x;
    const u64 mine = b < B ? load[b] | (drain[b] ? 1ull << 63 : 0) : 0;
    const int r = rank_ahead<kDkThreads, false, true>(B, b, mine, 1, load, nullptr, drain);
    if (b < B) {   // ranks are a permutation: r < B
        rank[b] = r;
        order[r] = b;
    }
}

// ... inside a count band: the plain rank, and the band's word of the broker from the count as it stands now, before the round's moves
__global__ __launch_bounds__(kDkThreads) void k_dk_rank_band(int B, const u64 *__restrict__ load, int32_t *__restrict__ rank, int32_t *__restrict__ order,
                                                             const int32_t *__restrict__ cnt, const uint8_t *__restrict__ rack, uint16_t *__restrict__ rf, int lo, int hi) {
    const int b = blockIdx.x * kDkThreads + threadIdx.x;
    const u64 mine = b < B ? load[b] : 0;
    const int r = rank_ahead<kDkThreads, false>(B, b, mine, 1, load, nullptr);
    if (b < B) {   // ranks are a permutation: r < B
        rank[b] = r;
        order[r] = b;
        const int c = cnt[b];
        rf[b] = (uint16_t)(rack[b] | (c >= hi ? kDkFull : 0) | (c <= lo ? kDkFloor : 0));
    }
}

// a row in registers: brokers, their racks (-1 in an empty slot), their ranks
struct DkRow {
    int b[KAO_MAX_RF], rk[KAO_MAX_RF], rr[KAO_MAX_RF];
};

__device__ __forceinline__ DkRow dk_load_row(const DkNet &n, int p) {
    const uint16_t *src = n.rows + (size_t)p * n.W;
    DkRow row;
#pragma unroll
    for (int j = 0; j < KAO_MAX_RF; ++j) {
        const int x = j < n.W ? (int)src[j] : (int)KAO_NONE;
        const bool held = x != KAO_NONE;
        row.b[j] = x;
        row.rk[j] = held ? (int)n.rack[x] : -1;
        row.rr[j] = held ? n.rank[x] : -1;
    }
    return row;
}

// c is admissible for a replica that leaves rack ra: not in the row; no rack rule, the same rack, or room in rack(c)
__device__ __forceinline__ bool dk_admissible(const DkRow &row, int c, int rc, int ra, int cap) {
    bool in_row = false;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < KAO_MAX_RF; ++j) {
        in_row |= row.b[j] == c;
        cnt += row.rk[j] == rc ? 1 : 0;
    }
    return !in_row && (cap <= 0 || rc == ra || cnt < cap);
}

// the input row in registers (under a budget only)
struct DkHome {
    int b[KAO_MAX_RF];
};

__device__ __forceinline__ DkHome dk_home_row(const DkNet &n, int p) {
    DkHome h;
    const uint16_t *src = n.rows0 + (size_t)p * n.W;
#pragma unroll
    for (int j = 0; j < KAO_MAX_RF; ++j) h.b[j] = j < n.W ? (int)src[j] : (int)KAO_NONE;
    return h;
}

__device__ __forceinline__ bool dk_home(const DkHome &h, int c) {   // c < KAO_NONE
    bool in = false;
#pragma unroll
    for (int j = 0; j < KAO_MAX_RF; ++j) in |= h.b[j] == c;
    return in;
}

// the gain test of a move a -> c.  By bytes: descent_gains.  By utilisation: (S(c) + w + min_gain) * cap(a) < S(a) * cap(c); S(c) + w
// stays below 2^63, and a sum that min_gain takes past 2^64 does not pass
template <bool Cap>
__device__ __forceinline__ bool dk_gains(const DkNet &n, u64 sa, u64 ca, int c, u64 w) {
    if (!Cap) return descent_gains(sa, n.load[c], w, n.min_gain);
    u64 left;
    if (__builtin_add_overflow(n.load[c] + w, n.min_gain, &left)) return false;
    return (u128)left * ca < (u128)sa * n.capacity[c];
}

// the first admissible broker among the ranks hi, hi - 1, .., lo; -1 when there is none.  Under a budget the broker must be
// affordable too: `free` (the size fits what is left, or the replica is a fresh copy), or a broker of the input row.  Gain (THOROUGH):
// it must pass the gain test by utilisation as well.  Band: the broker's band word stands in for its rack, and a full broker is passed over
template <bool Budget, bool Gain, bool Band = false, class Net = DkNet>
__device__ __forceinline__ int dk_walk(const Net &n, const DkRow &row, const DkHome &home, bool free, int hi, int lo, int ra, u64 sa = 0, u64 ca = 0, u64 w = 0) {
    for (int q = hi; q >= lo; --q) {
        const int c = n.order[q];
        if constexpr (Band) {
            const int word = n.rf[c];
            if (!(word & kDkFull) && dk_admissible(row, c, word & 0xFF, ra, n.cap)) return c;
        } else {
            if (dk_admissible(row, c, n.rack[c], ra, n.cap) && (!Budget || free || dk_home(home, c)) && (!Gain || dk_gains<true>(n, sa, ca, c, w))) return c;
        }
    }
    return -1;
}

// Drain: a slot on a broker of rank < n.nd is movable whatever its index and whatever the size, and proposes without a gain test; no walk
// goes below rank n.nd.  The other slots of a partition with size > 0 are as ever (with n.nd == 0 the proposals are those of <false>)
// Band: a slot on a broker at the band's floor is passed over (one word per slot tried), and the walks pass over the full brokers
template <bool Budget, bool Cap = false, bool Thorough = false, bool Drain = false, bool Band = false>
__global__ void k_dk_propose(std::conditional_t<Band, DkBandNet<DkNet>, DkNet> n, int r, uint32_t *__restrict__ count) {
    static_assert(!Drain || !(Budget || Cap || Thorough), "draining is by bytes, without a budget");
    static_assert(!Band || !(Budget || Cap || Thorough || Drain), "the count band is by bytes, without a budget or draining brokers");
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool prop = false;
    if (p < n.P) {
        u64 key = kDkNoKey;
        const u64 w = n.size[p];
        if constexpr (Drain) {
            const DkRow row = dk_load_row(n, p);
            const DkHome home{};
            const int lowest = w ? n.first : n.W;   // the lowest slot that is movable on a live broker
            int last = -1;
            for (int t = 0; t < n.W && !prop; ++t) {
                int ra_rank = n.B, a = 0, ra = 0, slot = 0;
#pragma unroll
                for (int j = 0; j < KAO_MAX_RF; ++j) {
                    if ((j >= lowest || row.rr[j] < n.nd) && row.rr[j] > last && row.rr[j] < ra_rank) { ra_rank = row.rr[j]; a = row.b[j]; ra = row.rk[j]; slot = j; }
                }
                if (ra_rank == n.B) break;   // no movable slot is left
                last = ra_rank;
                const bool leaves = ra_rank < n.nd;   // the source is draining
                int c = dk_walk<false, false>(n, row, home, true, n.B - 1 - ra_rank, max(ra_rank + 1, n.nd), ra);
                if (c < 0 || (!leaves && !descent_gains(n.load[a], n.load[c], w, n.min_gain))) {
                    c = dk_walk<false, false>(n, row, home, true, n.B - 1, max(n.B - ra_rank, n.nd), ra);
                    if (c >= 0 && !leaves && !descent_gains(n.load[a], n.load[c], w, n.min_gain)) c = -1;
                }
                if (c >= 0) {
                    prop = true;
                    key = (u64)(uint32_t)ra_rank << 48 | (u64)(0xFFFFu - wave_bytes_code(w)) << 32 | (u64)(uint32_t)p;
                    n.slot[p] = (uint8_t)slot;
                    n.dest[p] = (uint16_t)c;
                    u64 *mine = n.mk + (size_t)(r & 1) * n.B;
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&mine[a], key);
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&mine[c], key);
                }
            }
        } else if (w) {
            const DkRow row = dk_load_row(n, p);
            DkHome home;
            bool fits = true;   // the size fits what is left of the budget: tested first, so the home compares run only when it is nearly spent
            if (Budget) {
                home = dk_home_row(n, p);
                fits = w <= n.max_bytes - n.ctl[D_SPENT];
            }
            int last = -1;   // the rank of the slot tried before: ranks are distinct, so the slots come heaviest first
            for (int t = n.first; t < n.W && !prop; ++t) {
                int ra_rank = n.B, a = 0, ra = 0, slot = 0;
#pragma unroll
                for (int j = 0; j < KAO_MAX_RF; ++j) {
                    if (j >= n.first && row.rr[j] > last && row.rr[j] < ra_rank) { ra_rank = row.rr[j]; a = row.b[j]; ra = row.rk[j]; slot = j; }
                }
                if (ra_rank == n.B) break;   // no movable slot is left
                last = ra_rank;
                if constexpr (Band) {
                    if (n.rf[a] & kDkFloor) continue;   // n(a) <= count_lo: not movable
                }
                const u64 sa = n.load[a];
                const bool free = !Budget || fits || !dk_home(home, a);
                const u64 ca = Cap ? n.capacity[a] : 0;
                int c;
                if (Thorough) {
                    c = dk_walk<Budget, true>(n, row, home, free, n.B - 1, ra_rank + 1, ra, sa, ca, w);
                } else {
                    c = dk_walk<Budget, false, Band>(n, row, home, free, n.B - 1 - ra_rank, ra_rank + 1, ra);
                    if (c < 0 || !dk_gains<Cap>(n, sa, ca, c, w)) {
                        c = dk_walk<Budget, false, Band>(n, row, home, free, n.B - 1, n.B - ra_rank, ra);
                        if (c >= 0 && !dk_gains<Cap>(n, sa, ca, c, w)) c = -1;
                    }
                }
                if (c >= 0) {
                    prop = true;
                    key = (u64)(uint32_t)ra_rank << 48 | (u64)(0xFFFFu - wave_bytes_code(w)) << 32 | (u64)(uint32_t)p;
                    n.slot[p] = (uint8_t)slot;
                    n.dest[p] = (uint16_t)c;
                    u64 *mine = n.mk + (size_t)(r & 1) * n.B;
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&mine[a], key);
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&mine[c], key);
                }
            }
        }
        n.key[p] = key;
    }
    lane_count_to(prop, count);
}

// under a budget, between propose and apply: which winners are applied.  ONE workgroup walks the ranks q = 0, 1, ..; lane t of a chunk
// takes rank base + t.  b = order[q] is the source of a winner iff its minkey word carries rank q (a word with another rank is a
// proposal INTO b) and the destination's word holds the same key.  The charges get an exclusive u64 prefix sum over the ranks:
// shuffles inside a wavefront, the wavefront totals through LDS, a carry from chunk to chunk.  Sums stay below 2^62.
__global__ __launch_bounds__(kDkGrantThreads) void k_dk_grant(DkNet n, int r) {
    constexpr int kWaves = kDkGrantThreads / 64;
    __shared__ u64 wave_sum[kWaves];
    const u64 *mine = n.mk + (size_t)(r & 1) * n.B;
    const u64 rem = n.max_bytes - n.ctl[D_SPENT];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    u64 carry = 0;   // the charges of the chunks before this one
    for (int base = 0; base < n.B; base += kDkGrantThreads) {
        const int q = base + (int)threadIdx.x;
        bool win = false;
        u64 charge = 0;
        int b = 0;
        if (q < n.B) {
            b = n.order[q];
            const u64 key = mine[b];
            if (key != kDkNoKey && (int)(key >> 48) == q) {
                const uint32_t p = (uint32_t)key;   // a key of this round: p < P, slot[p] and dest[p] are this round's
                const int c = n.dest[p];
                if (mine[c] == key) {
                    win = true;
                    const uint16_t *was = n.rows0 + (size_t)p * n.W;
                    bool a_home = false, c_home = false;
                    for (int j = 0; j < n.W; ++j) {
                        a_home |= was[j] == b;
                        c_home |= was[j] == c;
                    }
                    charge = a_home && !c_home ? n.size[p] : 0;
                }
            }
        }
        u64 incl = charge;   // inclusive scan of the wavefront
        for (int off = 1; off < 64; off <<= 1) {
            const u64 up = (u64)__shfl_up((long long)incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        u64 before = carry, chunk = 0;   // the wavefronts below this one; the whole chunk
        for (int v = 0; v < kWaves; ++v) {
            const u64 x = wave_sum[v];
            before += v < wave ? x : 0;
            chunk += x;
        }
        __syncthreads();   // wave_sum is rewritten by the next chunk
        carry += chunk;
        const bool ok = win && (charge == 0 || before + incl <= rem);   // before + incl = the exclusive prefix + the own charge
        if (q < n.B) n.grant[b] = ok ? 1 : 0;
        lane_count_to(win && !ok, &n.ctl[D_REFUSED]);
    }
}

// ---- exchange rounds (kao_balance_disk_exchange) -----------------------------------------------------------------
// Where a round has no move proposal, two replicas of different partitions trade places across a broker pair (include/kao.h has the
// definition).  x walks the lighter brokers c lightest first; the partners y on c whose size lies in (size[x] - D + min_gain, size[x]),
// D = S(a) - S(c), pass; of those the one whose delta = size[x] - size[y] is nearest D / 2 is taken (the neighbours of the split
// 2 size[y] > 2 size[x] - D inside the passing run).  A proposal wins iff its key is the lowest at both brokers AND at both
// partitions: a partition has several replicas, so two winners at four distinct brokers could otherwise write one row.
// A type of its own: the kernels above keep their arguments.  PI (the partitions with size > 0, size descending, then index ascending)
// is sorted by the host once; bit t & 63 of mask[b * words + (t >> 6)] is set iff the partition at position t of PI has a movable slot on
// broker b.  k_dkx_index builds the masks from the input rows; k_dk_apply<false, true> keeps them current through rounds of BOTH kinds (a move
// flips two bits, an exchange four; a winner alone touches the mask rows of its two brokers), so no round rebuilds them.
struct DkNetX : DkNet {
    int N, words;              // positions of PI; mask words per broker
    const uint32_t *pi;        // [N] the partition at a position
    const u64 *ps;             // [N] its size: descending
    const uint32_t *pos;       // [P] the position of a partition (unset for size 0)
    u64 *mask;                 // [B * words]
    u64 *pk;                   // [2][P] minkey rows of the partitions: a partition named by two proposals, in either role, is won by one
    uint16_t *xsrc;            // [P] what the proposer of an exchange stores beside slot[] and dest[]: a,
    uint32_t *xpart;           // [P] the partner y,
    uint8_t *xslot;            // [P] and y's slot k on c.  APPLY reads these, never a row another winner may write
};

__global__ void k_dkx_index(DkNetX n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n.N) return;
    const uint16_t *row = n.rows0 + (size_t)n.pi[t] * n.W;
    for (int j = n.first; j < n.W; ++j) {
        const int b = row[j];
        if (b == KAO_NONE) break;
        atomicOr(&n.mask[(size_t)b * n.words + (t >> 6)], 1ull << (t & 63));
    }
}

// the first position in [lo, hi) whose size is <= lim (hi when there is none); sizes descend.  2 * size when Twice: both stay below 2^63
template <bool Twice>
__device__ __forceinline__ int dkx_first_le(const u64 *__restrict__ ps, int lo, int hi, long long lim) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const long long v = (long long)(Twice ? 2 * ps[mid] : ps[mid]);
        if (v <= lim) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the partner test of the partition at a position of c's mask: a is not in row y and the rack rule holds for the replica that leaves
// rack(c) for rack(a).  Returns y's slot on c, -1 when y is no partner
__device__ __forceinline__ int dkx_partner(const DkNetX &n, int y, int a, int c, int rka, int rkc) {
    const uint16_t *row = n.rows + (size_t)y * n.W;
    bool in_row = false;
    int cnt = 0, k = -1;
    for (int j = 0; j < n.W; ++j) {
        const int b = row[j];
        if (b == KAO_NONE) break;
        in_row |= b == a;
        cnt += (int)n.rack[b] == rka ? 1 : 0;
        if (b == c && j >= n.first) k = j;
    }
    return !in_row && (n.cap <= 0 || rka == rkc || cnt < n.cap) ? k : -1;
}

// the first position in [from, to) set in the mask row m whose partition is a partner (upward), the last one (downward); -1 without one.
// *k = the partner's slot
template <bool Up>
__device__ __forceinline__ int dkx_scan(const DkNetX &n, const u64 *__restrict__ m, int from, int to, int a, int c, int rka, int rkc, int *k) {
    if (from >= to) return -1;
    if (Up) {
        for (int wd = from >> 6; wd <= (to - 1) >> 6; ++wd) {
            u64 bits = m[wd];
            if (wd == from >> 6) bits &= ~0ull << (from & 63);
            while (bits) {
                const int t = wd * 64 + __ffsll((long long)bits) - 1;
                if (t >= to) return -1;
                if ((*k = dkx_partner(n, (int)n.pi[t], a, c, rka, rkc)) >= 0) return t;
                bits &= bits - 1;
            }
        }
    } else {
        for (int wd = (to - 1) >> 6; wd >= from >> 6; --wd) {
            u64 bits = m[wd];
            if (wd == (to - 1) >> 6) bits &= ~0ull >> (63 - ((to - 1) & 63));
            while (bits) {
                const int hi = 63 - __clzll((long long)bits), t = wd * 64 + hi;
                if (t < from) return -1;
                if ((*k = dkx_partner(n, (int)n.pi[t], a, c, rka, rkc)) >= 0) return t;
                bits &= ~(1ull << hi);
            }
        }
    }
    return -1;
}

// the EXCHANGE proposals of round r: nothing when the round has a move proposal (*count != 0) or the call has ended (ctl[D_DONE]: a
// round had neither kind).  One lane per partition x, the row in registers as in k_dk_propose.  Lane 0 of the grid notes the peak at
// the first exchange round: order[0] is the heaviest broker, and no load changes in this phase.
__global__ void k_dkx_propose(DkNetX n, int r, const uint32_t *__restrict__ count, uint32_t *__restrict__ xcount) {
    if (n.ctl[D_DONE] != 0 || *count != 0) return;   // (uniform over the grid)
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0 && n.ctl[D_XSEEN] == 0) {
        n.ctl[D_XSEEN] = 1;
        n.ctl[D_XPEAK] = n.load[n.order[0]];
    }
    bool prop = false;
    if (p < n.P) {
        const u64 w = n.size[p];
        if (w) {
            const DkRow row = dk_load_row(n, p);
            const int top = dkx_first_le<false>(n.ps, (int)n.pos[p], n.N, (long long)w - 1);   // delta > 0 from here on
            int last = -1;
            for (int t = n.first; t < n.W && !prop; ++t) {
                int ra_rank = n.B, a = 0, ra = 0, slot = 0;
#pragma unroll
                for (int j = 0; j < KAO_MAX_RF; ++j) {
                    if (j >= n.first && row.rr[j] > last && row.rr[j] < ra_rank) { ra_rank = row.rr[j]; a = row.b[j]; ra = row.rk[j]; slot = j; }
                }
                if (ra_rank == n.B) break;
                last = ra_rank;
                const u64 sa = n.load[a];
                int end = n.N;   // D only shrinks along the walk, and the end of the passing interval with it
                for (int q = n.B - 1; q > ra_rank; --q) {
                    const int c = n.order[q], rc = n.rack[c];
                    if (!dk_admissible(row, c, rc, ra, n.cap)) continue;
                    const u64 sc = n.load[c];
                    if (sa <= sc) continue;
                    const u64 D = sa - sc;
                    if (n.min_gain >= D) break;   // nothing passes here, nor at any later (heavier) c
                    end = dkx_first_le<false>(n.ps, top, end, (long long)w - (long long)(D - n.min_gain));   // size > size[x] - D + min_gain before it
                    if (end <= top) break;        // the passing interval holds no position of PI: none for a smaller D either
                    const int g = dkx_first_le<true>(n.ps, top, end, 2 * (long long)w - (long long)D);   // the split inside the passing run
                    const u64 *m = n.mask + (size_t)c * n.words;
                    int k_lo = -1, k_hi = -1;
                    const int t_lo = dkx_scan<true>(n, m, g, end, a, c, ra, rc, &k_lo), t_hi = dkx_scan<false>(n, m, top, g, a, c, ra, rc, &k_hi);
                    if (t_lo < 0 && t_hi < 0) continue;
                    bool take_lo = t_hi < 0;
                    if (t_lo >= 0 && t_hi >= 0) {   // |2 delta - D|: 2 delta >= D at y_lo, 2 delta < D at y_hi; a tie goes to y_lo
                        const u64 m_lo = 2 * (w - n.ps[t_lo]) - D, m_hi = D - 2 * (w - n.ps[t_hi]);
                        take_lo = m_lo <= m_hi;
                    }
                    const int ty = take_lo ? t_lo : t_hi;
                    const uint32_t y = n.pi[ty];
                    const u64 key = (u64)(uint32_t)ra_rank << 48 | (u64)(0xFFFFu - wave_bytes_code(w - n.ps[ty])) << 32 | (u64)(uint32_t)p;
                    prop = true;
                    n.key[p] = key;
                    n.slot[p] = (uint8_t)slot;
                    n.dest[p] = (uint16_t)c;
                    n.xsrc[p] = (uint16_t)a;
                    n.xpart[p] = y;
                    n.xslot[p] = (uint8_t)(take_lo ? k_lo : k_hi);
                    u64 *mine = n.mk + (size_t)(r & 1) * n.B, *part = n.pk + (size_t)(r & 1) * n.P;
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&mine[a], key);
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&mine[c], key);
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&part[p], key);
                    descent_bid<__HIP_MEMORY_SCOPE_AGENT>(&part[y], key);
                    break;
                }
            }
        }
    }
    lane_count_to(prop, xcount);
}

// the move that lane p proposed with `key`, if it won the round (mine = the round's minkey row): the lowest key at both of its
// brokers and, under a budget, granted.  No other winner touches a or c, and no other lane writes this row: plain stores.  The exchange
// call keeps its masks current (a move flips two bits).  *cost, under a budget: +size, 0 or -size (wrapping)
template <bool Budget, bool X, bool Band = false, class Net>
__device__ __forceinline__ bool dk_apply_move(const Net &n, int p, u64 key, const u64 *mine, u64 *cost) {
    uint16_t *row = n.rows + (size_t)p * n.W;
    const int slot = n.slot[p], a = row[slot], c = n.dest[p];
    bool won = mine[a] == key && mine[c] == key;
    if (Budget) won = won && n.grant[a] != 0;   // grant[] was settled from the spend before this kernel, which changes it
    if (won) {
        const u64 w = n.size[p];
        if (Budget) {
            const DkHome home = dk_home_row(n, p);
            *cost = (dk_home(home, c) ? 0 : w) - (dk_home(home, a) ? 0 : w);
        }
        n.load[a] -= w;
        n.load[c] += w;
        row[slot] = (uint16_t)c;
        if constexpr (Band) {
            n.cnt[a] -= 1;
            n.cnt[c] += 1;
        }
        if constexpr (X) {
            const uint32_t px = n.pos[p];
            const u64 bx = 1ull << (px & 63);
            n.mask[(size_t)a * n.words + (px >> 6)] &= ~bx;
            n.mask[(size_t)c * n.words + (px >> 6)] |= bx;
        }
    }
    return won;
}

// APPLY of round r.  It clears the minkey words of round r + 1 (last read by the apply of round r - 1) and applies the winners.  In
// the exchange call (X; count, xcount = the round's proposals of the two kinds) the round is whichever kind it is: an exchange round
// iff it has no move proposal, and ctl[D_DONE] is set once a round has had neither kind.  A winner of an exchange reads only what its
// proposer stored (an exchange flips four mask bits; a winner alone touches the mask rows of its two brokers).  Drain: a winner whose
// key carries a rank below n.nd left a draining broker; they are counted, and the last round (from 1) that had one is kept.  Band: the
// winner of a move also takes one off n(a) and adds one to n(c); an exchange keeps both.
template <bool Budget, bool X, bool Drain = false, bool Band = false>
__global__ void k_dk_apply(std::conditional_t<Band, DkBandNet<std::conditional_t<X, DkNetX, DkNet>>, std::conditional_t<X, DkNetX, DkNet>> n, int r,
                           const uint32_t *__restrict__ count, const uint32_t *__restrict__ xcount) {
    static_assert(!(Budget && X), "exchange rounds are by bytes, without a budget");
    static_assert(!Drain || !(Budget || X), "draining is by bytes, without a budget or exchanges");
    static_assert(!Band || !(Budget || Drain), "the count band is by bytes, without a budget or draining brokers");
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    {
        u64 *clr = n.mk + (size_t)((r + 1) & 1) * n.B;
        for (int e = p; e < n.B; e += gridDim.x * blockDim.x) clr[e] = kDkNoKey;
        if constexpr (X) {
            if (p < n.P) n.pk[(size_t)((r + 1) & 1) * n.P + p] = kDkNoKey;
        }
    }
    bool isx = false;   // the round is an exchange round
    if constexpr (X) {
        isx = *count == 0;
        if (p == 0 && isx && *xcount == 0) n.ctl[D_DONE] = 1;
    }
    bool won = false, left = false;   // left: the winner took a replica off a draining broker
    u64 cost = 0;
    if (p < n.P) {
        const u64 key = n.key[p];
        if (key != kDkNoKey) {
            const u64 *mine = n.mk + (size_t)(r & 1) * n.B;
            if (!isx) {
                won = dk_apply_move<Budget, X, Band>(n, p, key, mine, &cost);
                if (Drain) left = won && (int)(key >> 48) < n.nd;
            } else if constexpr (X) {
                const int slot = n.slot[p], a = n.xsrc[p], c = n.dest[p];
                const uint32_t y = n.xpart[p];
                const u64 *part = n.pk + (size_t)(r & 1) * n.P;
                won = mine[a] == key && mine[c] == key && part[p] == key && part[y] == key;
                if (won) {   // no other winner touches a, c, x or y
                    const u64 d = n.size[p] - n.size[y];
                    const uint32_t px = n.pos[p], py = n.pos[y];
                    const u64 bx = 1ull << (px & 63), by = 1ull << (py & 63);
                    u64 *ma = n.mask + (size_t)a * n.words, *mc = n.mask + (size_t)c * n.words;
                    n.load[a] -= d;
                    n.load[c] += d;
                    n.rows[(size_t)p * n.W + slot] = (uint16_t)c;
                    n.rows[(size_t)y * n.W + n.xslot[p]] = (uint16_t)a;
                    ma[px >> 6] &= ~bx;
                    ma[py >> 6] |= by;
                    mc[px >> 6] |= bx;
                    mc[py >> 6] &= ~by;
                }
            }
        }
    }
    lane_count_to(won, &n.ctl[D_MOVES]);
    if (Budget) wave_sum_to(cost, &n.ctl[D_SPENT]);   // the sum of a wavefront wraps as its terms do; it adds nothing when it is 0
    if constexpr (X) lane_count_to(won && isx, &n.ctl[D_XCH]);
    if constexpr (Drain) {
        lane_count_to(left, &n.ctl[D_DRAINED]);
        wave_max_to(left ? (u64)r + 1 : 0, &n.ctl[D_LASTDRAIN]);
    }
}

// ---- the result ---------------------------------------------------------------------------------------------------------------------
// one lane per partition: the brokers of the final row that the input row did not hold, their bytes, the rows that changed.  Drain:
// and the replicas still on draining brokers, with their bytes
template <bool Drain>
__global__ void k_dk_finish(DkNet n) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    bool ch = false;
    u64 fresh = 0, bytes = 0, stay = 0;
    if (p < n.P) {
        const uint16_t *now = n.rows + (size_t)p * n.W, *was = n.rows0 + (size_t)p * n.W;
        for (int j = 0; j < n.W; ++j) {
            const int x = now[j];
            if (x == KAO_NONE) break;
            ch |= x != was[j];
            bool old = false;
            for (int i = 0; i < n.W; ++i) old |= was[i] == x;
            fresh += old ? 0 : 1;
            if (Drain) stay += n.drain[x] ? 1 : 0;
        }
        bytes = fresh * n.size[p];
    }
    if constexpr (Drain) {
        wave_sum_to(stay, &n.ctl[D_NLEFT]);
        wave_sum_to(p < n.P ? stay * n.size[p] : 0, &n.ctl[D_BLEFT]);
    }
    wave_sum_to(fresh, &n.ctl[D_NMOVED]);
    wave_sum_to(bytes, &n.ctl[D_BYTES]);
    lane_count_to(ch, &n.ctl[D_ROWS]);
}

// the peak after; the brokers whose load changed
__device__ __forceinline__ void dk_peak1(const DkNet &n, const u64 *load0) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    u64 s = 0;
    bool ch = false;
    if (b < n.B) {
        s = n.load[b];
        ch = s != load0[b];
    }
    wave_max_to(s, &n.ctl[D_PEAK1]);
    lane_count_to(ch, &n.ctl[D_BROKERS]);
}

__global__ void k_dk_peak1(DkNet n, const u64 *__restrict__ load0) { dk_peak1(n, load0); }
__global__ void k_dk_peak1_band(DkBandNet<DkNet> n, const u64 *__restrict__ load0) {
    dk_peak1(n, load0);
    dk_count_range(n, blockIdx.x * blockDim.x + threadIdx.x, D_CMIN1, D_OUT1);
}

int validate_disk(const std::string &fn, int32_t B, int32_t R, const uint8_t *rack_of, int32_t P, int32_t W, const uint16_t *rows, const uint64_t *size,
                  const void *const *outs, int n_outs) {
    bool null = !rack_of || !rows || !size;
    for (int i = 0; i < n_outs; ++i) null |= !outs[i];
    if (null) return fail(KAO_ERR_INVALID, fn + "null pointer");
    int rc = check_dims(fn, B, P, W, R);
    if (!rc) rc = check_slot_cap(fn, P, W);
    if (rc) return rc;
    if (B > KAO_DISK_MAX_BROKERS) return fail(KAO_ERR_UNSUPPORTED, fn + "more than " + std::to_string(KAO_DISK_MAX_BROKERS) + " brokers (every round ranks all pairs of them)");
    for (int b = 0; b < B; ++b)
        if (rack_of[b] >= R) return fail(KAO_ERR_INVALID, fn + "rack_of[" + std::to_string(b) + "] >= n_racks");
    if ((rc = check_rows(fn, B, P, W, rows))) return rc;
    uint64_t total = 0;   // sum k_p size[p] below 2^62: every load of the kernels stays below 2^63
    for (int64_t p = 0; p < P; ++p) {
        uint64_t k = 0, all = 0;
        while (k < (uint64_t)W && rows[p * W + (int64_t)k] != KAO_NONE) ++k;
        if (__builtin_mul_overflow(k, size[p], &all) || __builtin_add_overflow(total, all, &total) || total >= (uint64_t(1) << 62))
            return fail(KAO_ERR_INVALID, fn + "partition " + std::to_string(p) + ": the replica sizes sum to 2^62 or more");
    }
    return KAO_OK;
}

// a fraction {numerator, denominator}, compared by the two 128-bit products; every part stays below 2^62 (denominators are >= 1)
struct DkFrac {
    uint64_t num, den;
};
bool frac_above(const DkFrac &x, const DkFrac &y) { return (u128)x.num * y.den > (u128)y.num * x.den; }
bool frac_equal(const DkFrac &x, const DkFrac &y) { return (u128)x.num * y.den == (u128)y.num * x.den; }

// {v[b], cap[b]} of the broker with the highest ratio, the lowest index on ties
DkFrac frac_peak(const std::vector<uint64_t> &v, const uint64_t *cap) {
    size_t at = 0;
    for (size_t b = 1; b < v.size(); ++b)
        if (frac_above({v[b], cap[b]}, {v[at], cap[at]})) at = b;
    return {v[at], cap[at]};
}

// the integrality test: the sum over b of ceil(S* cap(b) / cap*) - 1 is below `total`, so no placement puts every broker strictly
// below the utilisation S* / cap*.  (S* == 0 only when total == 0, and then the peak equals the bound.)
bool frac_integral(const DkFrac &peak, const uint64_t *cap, int B, uint64_t total) {
    if (peak.num == 0) return false;
    u128 sum = 0;
    for (int b = 0; b < B && sum < total; ++b) sum += ((u128)peak.num * cap[b] + peak.den - 1) / peak.den - 1;   // each term >= 0: the product is >= 1
    return sum < total;
}

// ---- the host side of a call ----------------------------------------------------------------------------------------------------------
// Which entry point: budget adds k_dk_grant to every round, stats[8], stats[9] and the probe that decides stats[9]; cap (by utilisation)
// the rank by utilisation, the capacity form of the test, THOROUGH rounds, fractions as outputs and stats[10]; exchange
// (kao_balance_disk_exchange: by bytes, without a budget, as k_dk_apply asserts) PI, the masks and the partition words, the exchange
// PROPOSE in every round (it returns at once in a round with a move proposal, and after the call has ended) and stats[8..11]; drain
// (kao_balance_disk_drain: by bytes, without a budget or exchanges) the drain forms of RANK, PROPOSE, APPLY, the init and the finish, the
// bound over the live brokers, n_left / bytes_left and stats[8..9].  It launches what kao_balance_disk launches, kernel for kernel.  band
// (kao_balance_disk_banded: by bytes, without a budget or draining, with or without exchange) the band forms of INIT, RANK, PROPOSE, APPLY
// and the two peaks, the counts, count_range and stats[12..13]; again kernel for kernel what the call without a band launches.
struct DkKind {
    bool budget, cap, exchange, drain = false, band = false;
};

struct DkArgs {   // the arguments of the C calls in their order (cap, max_bytes where the call has them); the peaks and the bound are two words by utilisation
    int32_t B, R; const uint8_t *rack_of; int32_t P, W; uint16_t *rows; const uint64_t *size, *cap;
    int32_t max_per_rack, move_leaders; uint64_t min_gain, max_bytes; int32_t max_rounds, dry_run;
    int32_t *n_moved; uint64_t *bytes_moved, *peak_before, *peak_after, *lower_bound; int32_t *status; int64_t *stats;
    const uint8_t *drain = nullptr; int32_t *n_left = nullptr; uint64_t *bytes_left = nullptr;   // kao_balance_disk_drain only
    int32_t count_lo = 0, count_hi = 0, *count_range = nullptr;                                  // kao_balance_disk_banded only
};

struct DkCall {   // one call on the host
    DkKind kind;
    uint64_t cap_sum = 0, cap_max = 0;   // by utilisation
    std::vector<uint32_t> pi, pos;       // exchange: PI (the partitions with size > 0, size descending, then index ascending), the position of
    std::vector<uint64_t> ps;            // a partition in it, the sizes along it
    int n_drain = 0;                     // draining: D
    CallBufs m;
    hipStream_t st;
    DkNetX x;                 // the exchange call's; its DkNet part is every call's
    uint32_t *d_cnt;          // [2][kDkBatch] the move proposals of a batch's rounds, then (exchange) their exchange proposals
    u64 *d_fixed, *d_load0;   // [B] the bytes of the slot-0 replicas; the loads of the input
    int32_t *d_n = nullptr, lo = 0, hi = 0;   // inside a count band: [B] n(b); the band
    uint16_t *d_rf = nullptr;                 // ... [B] the band words of the round
    template <class Base>
    DkBandNet<Base> banded(const Base &net) const {   // the net a band kernel takes
        DkBandNet<Base> b;
        static_cast<Base &>(b) = net;
        b.cnt = d_n; b.rf = d_rf; b.lo = lo; b.hi = hi;
        return b;
    }
    unsigned pblocks, bblocks;
    int64_t launches = 0, rounds = 0, props = 0, thorough_rounds = 0, x_rounds = 0, x_props = 0;   // what the host counts
    bool more = false, open = false;   // max_rounds rounds have run and there is more to do; the budget stopped the descent
    const DkNet &n() const { return x; }
};

// 1 <= cap[b], and a sum below 2^62: with the loads below 2^62 every product of the two fits 128 bits
int dk_check_capacity(const std::string &fn, int B, const uint64_t *cap, DkCall &c) {
    for (int b = 0; b < B; ++b) {
        if (cap[b] == 0) return fail(KAO_ERR_INVALID, fn + "cap[" + std::to_string(b) + "] is 0");
        if (__builtin_add_overflow(c.cap_sum, cap[b], &c.cap_sum) || c.cap_sum >= (uint64_t(1) << 62))
            return fail(KAO_ERR_INVALID, fn + "cap[" + std::to_string(b) + "]: the capacities sum to 2^62 or more");
        c.cap_max = std::max(c.cap_max, cap[b]);
    }
    return KAO_OK;
}

// the exchange call's order: a host sort, once (the sizes never change)
int dkx_build_order(const std::string &fn, int B, int P, const uint64_t *size, DkCall &o) {
    for (int32_t p = 0; p < P; ++p)
        if (size[p]) o.pi.push_back((uint32_t)p);
    if ((uint64_t)B * ((o.pi.size() + 63) / 64) > KAO_DISK_EXCHANGE_MAX_WORDS)
        return fail(KAO_ERR_UNSUPPORTED, fn + "n_brokers * ceil(N / 64) is above 2^27 mask words (N = the partitions with size > 0)");
    std::sort(o.pi.begin(), o.pi.end(), [&](uint32_t x, uint32_t y) { return size[x] != size[y] ? size[x] > size[y] : x < y; });
    o.pos.assign((size_t)P, 0);
    o.ps.resize(o.pi.size());
    for (size_t t = 0; t < o.pi.size(); ++t) {
        o.pos[o.pi[t]] = (uint32_t)t;
        o.ps[t] = size[o.pi[t]];
    }
    return KAO_OK;
}

// carves the arena, uploads the inputs and fills the net; with exchange it builds the masks (k_dkx_index)
int dk_open(DkCall &c, const DkArgs &in) {
    const bool X = c.kind.exchange;
    const int B = in.B, P = in.P, PW = P * in.W, N = (int)c.pi.size(), words = (N + 63) / 64;
    // one arena: ctl u64[D_N] | count u32[2 kDkBatch] | load, fixed u64[B] | n i32[B] (band; zeroed up to here) | rf u16[B] (band) | mk u64[2B] (all ones) | load0 u64[B] | capacity u64[B] |
    //            rank, order i32[B] | key, size u64[P] | rows, rows0 u16[PW] | dest u16[P] | slot u8[P] | rack u8[B] | grant u8[B] | drain u8[B]
    Carve cv;
    const size_t o_ctl = cv.take<u64>(D_N), o_cnt = cv.take<uint32_t>(2 * kDkBatch), o_load = cv.take<u64>(B), o_fixed = cv.take<u64>(B),
                 o_n = cv.take<int32_t>(c.kind.band ? B : 0), zeroed = cv.end(), o_rf = cv.take<uint16_t>(c.kind.band ? B : 0), o_mk = cv.take<u64>(2 * (size_t)B), o_load0 = cv.take<u64>(B), o_cap = cv.take<u64>(c.kind.cap ? B : 0), o_rank = cv.take<int32_t>(B),
                 o_order = cv.take<int32_t>(B), o_key = cv.take<u64>(P), o_size = cv.take<u64>(P), o_rows = cv.take<uint16_t>(PW),
                 o_rows0 = cv.take<uint16_t>(PW), o_dest = cv.take<uint16_t>(P), o_slot = cv.take<uint8_t>(P), o_rack = cv.take<uint8_t>(B),
                 o_grant = cv.take<uint8_t>(c.kind.budget ? B : 0), o_drain = cv.take<uint8_t>(c.kind.drain ? B : 0);
    // exchange: pk u64[2P] (all ones) | mask u64[B words] (zeroed) | ps u64[N] | pi u32[N] | pos, xpart u32[P] | xsrc u16[P] | xslot u8[P]
    const size_t o_pk = cv.take<u64>(X ? 2 * (size_t)P : 0), o_mask = cv.take<u64>(X ? (size_t)B * words : 0), o_ps = cv.take<u64>(N), o_pi = cv.take<uint32_t>(N),
                 o_pos = cv.take<uint32_t>(X ? P : 0), o_xpart = cv.take<uint32_t>(X ? P : 0), o_xsrc = cv.take<uint16_t>(X ? P : 0),
                 o_xslot = cv.take<uint8_t>(X ? P : 0);
    if (int rc = c.m.open(cv.end())) return rc;
    const CallBufs &m = c.m;
    hipStream_t st = c.st = m.stream;
    c.d_cnt = m.at<uint32_t>(o_cnt); c.d_fixed = m.at<u64>(o_fixed); c.d_load0 = m.at<u64>(o_load0);
    c.d_n = m.at<int32_t>(o_n); c.d_rf = m.at<uint16_t>(o_rf); c.lo = in.count_lo; c.hi = in.count_hi;
    c.pblocks = grid_for(P, kDkThreads); c.bblocks = grid_for(B, kDkThreads);
    DkNetX &n = c.x;
    n.P = P; n.W = in.W; n.B = B; n.cap = in.max_per_rack; n.first = in.move_leaders ? 0 : 1; n.min_gain = in.min_gain;
    n.rows = m.at<uint16_t>(o_rows); n.rows0 = m.at<uint16_t>(o_rows0); n.size = m.at<u64>(o_size); n.rack = m.at<uint8_t>(o_rack);
    n.slot = m.at<uint8_t>(o_slot); n.dest = m.at<uint16_t>(o_dest); n.key = m.at<u64>(o_key); n.load = m.at<u64>(o_load);
    n.rank = m.at<int32_t>(o_rank); n.order = m.at<int32_t>(o_order); n.mk = m.at<u64>(o_mk); n.ctl = m.at<u64>(o_ctl);
    n.grant = m.at<uint8_t>(o_grant); n.max_bytes = in.max_bytes; n.capacity = c.kind.cap ? m.at<u64>(o_cap) : nullptr;
    n.nd = c.n_drain; n.drain = c.kind.drain ? m.at<uint8_t>(o_drain) : nullptr;
    n.N = N; n.words = words; n.pi = m.at<uint32_t>(o_pi); n.ps = m.at<u64>(o_ps); n.pos = m.at<uint32_t>(o_pos); n.mask = m.at<u64>(o_mask);
    n.pk = m.at<u64>(o_pk); n.xsrc = m.at<uint16_t>(o_xsrc); n.xpart = m.at<uint32_t>(o_xpart); n.xslot = m.at<uint8_t>(o_xslot);

    HIP_TRY(hipMemsetAsync(m.arena, 0, zeroed, st));
    HIP_TRY(hipMemsetAsync(n.mk, 0xFF, 2 * (size_t)B * sizeof(u64), st));
    HIP_TRY(hipMemcpyAsync(m.at<uint8_t>(o_rack), in.rack_of, (size_t)B, hipMemcpyHostToDevice, st));
    if (P) {
        HIP_TRY(hipMemcpyAsync(m.at<uint16_t>(o_rows0), in.rows, (size_t)PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(n.rows, n.rows0, (size_t)PW * sizeof(uint16_t), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<u64>(o_size), in.size, (size_t)P * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    }
    if (c.kind.cap) HIP_TRY(hipMemcpyAsync(m.at<u64>(o_cap), in.cap, (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (c.kind.drain) HIP_TRY(hipMemcpyAsync(m.at<uint8_t>(o_drain), in.drain, (size_t)B, hipMemcpyHostToDevice, st));
    if (X && P) {
        HIP_TRY(hipMemsetAsync(n.pk, 0xFF, 2 * (size_t)P * sizeof(u64), st));
        HIP_TRY(hipMemcpyAsync(m.at<uint32_t>(o_pos), c.pos.data(), (size_t)P * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if (X && N) {
        HIP_TRY(hipMemsetAsync(n.mask, 0, (size_t)B * words * sizeof(u64), st));
        HIP_TRY(hipMemcpyAsync(m.at<uint32_t>(o_pi), c.pi.data(), (size_t)N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(m.at<u64>(o_ps), c.ps.data(), (size_t)N * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        k_dkx_index<<<grid_for(N, kDkThreads), kDkThreads, 0, st>>>(n);
        ++c.launches;
    }
    return KAO_OK;
}

// PROPOSE: by bytes, or FAST / THOROUGH by utilisation; `budget` is the round's (the probe at the end of a budgeted call runs without)
void dk_propose(const DkCall &c, bool budget, bool thorough, int r, uint32_t *count) {
    if (c.kind.band) {
        k_dk_propose<false, false, false, false, true><<<c.pblocks, kDkThreads, 0, c.st>>>(c.banded(c.n()), r, count);
        return;
    }
    void (*const k)(DkNet, int, uint32_t *) = c.kind.drain ? k_dk_propose<false, false, false, true>
                                              : !c.kind.cap ? (budget ? k_dk_propose<true, false, false> : k_dk_propose<false, false, false>)
                                              : thorough  ? (budget ? k_dk_propose<true, true, true> : k_dk_propose<false, true, true>)
                                                          : (budget ? k_dk_propose<true, true, false> : k_dk_propose<false, true, false>);
    k<<<c.pblocks, kDkThreads, 0, c.st>>>(c.n(), r, count);
}

// APPLY of round r, whose proposals were counted in column i
void dk_apply(const DkCall &c, int r, int i) {
    if (c.kind.band && c.kind.exchange) k_dk_apply<false, true, false, true><<<c.pblocks, kDkThreads, 0, c.st>>>(c.banded(c.x), r, c.d_cnt + i, c.d_cnt + kDkBatch + i);
    else if (c.kind.band) k_dk_apply<false, false, false, true><<<c.pblocks, kDkThreads, 0, c.st>>>(c.banded(c.n()), r, nullptr, nullptr);
    else if (c.kind.exchange) k_dk_apply<false, true><<<c.pblocks, kDkThreads, 0, c.st>>>(c.x, r, c.d_cnt + i, c.d_cnt + kDkBatch + i);
    else if (c.kind.budget) k_dk_apply<true, false><<<c.pblocks, kDkThreads, 0, c.st>>>(c.n(), r, nullptr, nullptr);
    else if (c.kind.drain) k_dk_apply<false, false, true><<<c.pblocks, kDkThreads, 0, c.st>>>(c.n(), r, nullptr, nullptr);
    else k_dk_apply<false, false><<<c.pblocks, kDkThreads, 0, c.st>>>(c.n(), r, nullptr, nullptr);
}

// RANK, PROPOSE and (exchange) the exchange PROPOSE of round r, counted in column i: the head of a round, or all of "is there a proposal?"
void dk_probe(DkCall &c, bool budget, bool thorough, int r, int i) {
    const DkNet &n = c.n();
    if (c.kind.band) k_dk_rank_band<<<c.bblocks, kDkThreads, 0, c.st>>>(n.B, n.load, n.rank, n.order, c.d_n, n.rack, c.d_rf, c.lo, c.hi);
    else if (c.kind.drain) k_dk_rank_drain<<<c.bblocks, kDkThreads, 0, c.st>>>(n.B, n.load, n.drain, n.rank, n.order);
    else (c.kind.cap ? k_dk_rank<true> : k_dk_rank<false>)<<<c.bblocks, kDkThreads, 0, c.st>>>(n.B, n.load, n.capacity, n.rank, n.order);
    dk_propose(c, budget, thorough, r, c.d_cnt + i);
    c.launches += 2;
    if (c.kind.exchange) {
        k_dkx_propose<<<c.pblocks, kDkThreads, 0, c.st>>>(c.x, r, c.d_cnt + i, c.d_cnt + kDkBatch + i);
        ++c.launches;
    }
}

// the rounds, in batches: nb rounds are enqueued, then the host reads their proposal counts.  The rounds of a batch before the first
// one without a proposal of either kind ran; the ones after it changed nothing.  A budgeted call ends with the probe behind stats[9]
int dk_rounds(const std::string &fn, DkCall &c, int max_rounds) {
    uint32_t cnt[2 * kDkBatch] = {};   // the second row stays 0 without exchange
    bool thorough = false;             // by utilisation: a FAST round had no proposal
    for (int r = 0, done = 0; !done;) {
        if (r >= kDkHardRounds) return fail(KAO_ERR_HIP, fn + "the rounds did not finish");
        const int batch = thorough ? kDkThoroughBatch : kDkBatch;
        const int nb = max_rounds > 0 ? std::min(batch, max_rounds - r) : batch;
        HIP_TRY(hipMemsetAsync(c.d_cnt, 0, sizeof cnt, c.st));
        if (nb == 0) dk_probe(c, c.kind.budget, c.kind.cap, r, 0);   // max_rounds rounds have run, every one with a proposal: is there more to do?  (THOROUGH sees every move a FAST round sees)
        for (int i = 0; i < nb; ++i) {
            dk_probe(c, c.kind.budget, thorough, r + i, i);
            if (c.kind.budget) k_dk_grant<<<1, kDkGrantThreads, 0, c.st>>>(c.n(), r + i);
            dk_apply(c, r + i, i);
            c.launches += c.kind.budget ? 2 : 1;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt, c.d_cnt, sizeof cnt, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        if (nb == 0) { c.more = cnt[0] != 0 || cnt[kDkBatch] != 0; break; }
        int ran = 0;
        for (; ran < nb && (cnt[ran] != 0 || cnt[kDkBatch + ran] != 0); ++ran) {
            c.props += cnt[ran] + cnt[kDkBatch + ran];
            c.x_props += cnt[kDkBatch + ran];
            c.x_rounds += cnt[ran] == 0;   // a round without a move proposal is an exchange round
        }
        c.rounds += ran;
        if (thorough) c.thorough_rounds += ran;
        if (ran < nb && c.kind.cap && !thorough) {   // the first empty FAST round: THOROUGH from here on.  It and the empty rounds behind it left
            thorough = true;                         // both minkey rows clear and every key[p] empty, so the count of rounds goes on from `ran`
            r += ran;
        } else {
            done = ran < nb;                         // the first round without a proposal ends the descent
            r += nb;
        }
    }
    if (c.kind.budget && !c.more) {   // no affordable proposal is left: is there one without the budget?  (Round index 0; nothing is applied)
        HIP_TRY(hipMemsetAsync(c.d_cnt, 0, sizeof cnt[0], c.st));
        dk_probe(c, false, c.kind.cap, 0, 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt, c.d_cnt, sizeof cnt[0], hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        c.open = cnt[0] != 0;
    }
    return KAO_OK;
}

// the peaks, the bound (the highest of three terms, the lowest term on ties) and the status, by bytes; returns the term.  live = the
// brokers that share the bytes: all of them, or (draining) the ones that stay, and then the peak is proven only with nothing left
int dk_outputs_bytes(const u64 *ctl, const DkArgs &out, int live) {
    const uint64_t terms[3] = {(uint64_t)ctl[D_MAXSIZE], ((uint64_t)ctl[D_TOTAL] + (uint64_t)live - 1) / (uint64_t)live, out.move_leaders ? 0 : (uint64_t)ctl[D_FIXED]};
    int which = 0;
    for (int i = 1; i < 3; ++i)
        if (terms[i] > terms[which]) which = i;
    *out.peak_before = ctl[D_PEAK0];
    *out.peak_after = ctl[D_PEAK1];
    *out.lower_bound = terms[which];
    *out.status = ctl[D_PEAK1] == terms[which] && ctl[D_NLEFT] == 0 ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
    return which;
}

// ... by utilisation: fractions, their maxima taken on the host from h = load0, load, fixed; term 3 is the integrality test
int dk_outputs_fractions(const u64 *ctl, const DkCall &c, const DkArgs &out, const std::vector<uint64_t> *h) {
    const uint64_t *cap = out.cap;
    const DkFrac terms[3] = {{(uint64_t)ctl[D_MAXSIZE], c.cap_max}, {(uint64_t)ctl[D_TOTAL], c.cap_sum}, out.move_leaders ? DkFrac{0, 1} : frac_peak(h[2], cap)};
    int which = 0;
    for (int i = 1; i < 3; ++i)
        if (frac_above(terms[i], terms[which])) which = i;
    const DkFrac before = frac_peak(h[0], cap), after = frac_peak(h[1], cap);
    out.peak_before[0] = before.num; out.peak_before[1] = before.den;
    out.peak_after[0] = after.num; out.peak_after[1] = after.den;
    out.lower_bound[0] = terms[which].num; out.lower_bound[1] = terms[which].den;
    bool proven = frac_equal(after, terms[which]);
    if (!proven && frac_integral(after, cap, out.B, (uint64_t)ctl[D_TOTAL])) { proven = true; which = 3; }
    *out.status = proven ? KAO_STATUS_OPTIMAL_PROVEN : KAO_STATUS_FEASIBLE_BOUND_GAP;
    return which;
}

int balance_disk(DkKind kind, const std::string &fn, const DkArgs &a) {
    if (kind.exchange && (kind.budget || kind.cap)) return fail(KAO_ERR_INVALID, fn + "exchange rounds are by bytes, without a budget");
    if (kind.drain && (kind.budget || kind.cap || kind.exchange)) return fail(KAO_ERR_INVALID, fn + "draining is by bytes, without a budget or exchanges");
    if (kind.band && (kind.budget || kind.cap || kind.drain)) return fail(KAO_ERR_INVALID, fn + "the count band is by bytes, without a budget or draining brokers");
    const void *outs[] = {a.n_moved, a.bytes_moved, a.peak_before, a.peak_after, a.lower_bound, a.status, a.drain, a.n_left, a.bytes_left};   // the last three: draining only
    int rc = validate_disk(fn, a.B, a.R, a.rack_of, a.P, a.W, a.rows, a.size, outs, kind.drain ? 9 : 6);
    if (rc) return rc;
    if (kind.band) {
        if (!a.count_range) return fail(KAO_ERR_INVALID, fn + "null pointer");
        if (a.count_lo < 0) return fail(KAO_ERR_INVALID, fn + "count_lo < 0");
        if (a.count_hi < a.count_lo) return fail(KAO_ERR_INVALID, fn + "count_hi < count_lo");
    }
    DkCall c;
    c.kind = kind;
    if (kind.drain) {
        for (int b = 0; b < a.B; ++b) c.n_drain += a.drain[b] != 0;
        if (c.n_drain == a.B) return fail(KAO_ERR_INVALID, fn + "every broker is draining: no live broker is left");
    }
    if (kind.cap && (rc = dk_check_capacity(fn, a.B, a.cap, c))) return rc;
    if (kind.exchange && (rc = dkx_build_order(fn, a.B, a.P, a.size, c))) return rc;
    if ((rc = require_init())) return rc;
    if ((rc = dk_open(c, a))) return rc;
    const DkNet &n = c.n();
    const int B = a.B, P = a.P;
    hipStream_t st = c.st;
    if (P) {
        if (kind.band) k_dk_init_band<<<c.pblocks, kDkThreads, 0, st>>>(c.banded(n), c.d_fixed);
        else (kind.drain ? k_dk_init<true> : k_dk_init<false>)<<<c.pblocks, kDkThreads, 0, st>>>(n, c.d_fixed);
        ++c.launches;
    }
    if (kind.band) k_dk_peak0_band<<<c.bblocks, kDkThreads, 0, st>>>(c.banded(n), c.d_fixed, c.d_load0);
    else k_dk_peak0<<<c.bblocks, kDkThreads, 0, st>>>(n, c.d_fixed, c.d_load0);
    ++c.launches;
    HIP_TRY(hipGetLastError());
    if (P) {
        if ((rc = dk_rounds(fn, c, a.max_rounds))) return rc;
        (kind.drain ? k_dk_finish<true> : k_dk_finish<false>)<<<c.pblocks, kDkThreads, 0, st>>>(n);
        ++c.launches;
    }
    if (kind.band) k_dk_peak1_band<<<c.bblocks, kDkThreads, 0, st>>>(c.banded(n), c.d_load0);
    else k_dk_peak1<<<c.bblocks, kDkThreads, 0, st>>>(n, c.d_load0);
    ++c.launches;
    HIP_TRY(hipGetLastError());
    u64 ctl[D_N];
    std::vector<uint64_t> h[3];   // by utilisation: load0, load, fixed.  A maximum over fractions is taken on the host, from one read at the end
    const u64 *d_h[3] = {c.d_load0, n.load, c.d_fixed};
    HIP_TRY(hipMemcpyAsync(ctl, n.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    for (int i = 0; kind.cap && i < 3; ++i) {
        h[i].resize(B);
        HIP_TRY(hipMemcpyAsync(h[i].data(), d_h[i], (size_t)B * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    }
    if (P && !a.dry_run) HIP_TRY(hipMemcpyAsync(a.rows, n.rows, (size_t)P * a.W * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    *a.n_moved = (int32_t)ctl[D_NMOVED];
    *a.bytes_moved = ctl[D_BYTES];
    const int which = kind.cap ? dk_outputs_fractions(ctl, c, a, h) : dk_outputs_bytes(ctl, a, B - c.n_drain);
    if (kind.drain) {
        *a.n_left = (int32_t)ctl[D_NLEFT];
        *a.bytes_left = ctl[D_BLEFT];
    }
    if (kind.band) {   // {min, max} of n(b) before, then after
        const u64 range[4] = {kDkCountTop - ctl[D_CMIN0], ctl[D_CMAX0], kDkCountTop - ctl[D_CMIN1], ctl[D_CMAX1]};
        for (int i = 0; i < 4; ++i) a.count_range[i] = (int32_t)range[i];
    }
    if (int64_t *stats = a.stats) {
        stats[0] = c.rounds; stats[1] = (int64_t)ctl[D_MOVES]; stats[2] = c.props; stats[3] = c.launches; stats[4] = (int64_t)ctl[D_ROWS];
        stats[5] = c.more ? 1 : 0; stats[6] = which; stats[7] = (int64_t)ctl[D_BROKERS];
        if (kind.band) {
            for (int i = 8; i < 12; ++i) stats[i] = 0;
            stats[12] = (int64_t)ctl[D_OUT1]; stats[13] = (int64_t)ctl[D_OUT0];
        }
        if (kind.exchange) {
            stats[8] = c.x_rounds; stats[9] = (int64_t)ctl[D_XCH]; stats[10] = c.x_props; stats[11] = (int64_t)ctl[D_XPEAK];
        } else if (kind.drain) {
            stats[8] = (int64_t)ctl[D_DRAINED]; stats[9] = (int64_t)ctl[D_LASTDRAIN];
        } else if (kind.budget || kind.cap) {   // by utilisation without a budget: both 0
            stats[8] = kind.budget ? (int64_t)ctl[D_REFUSED] : 0; stats[9] = c.open ? 1 : 0;
            if (kind.cap) stats[10] = c.thorough_rounds;
        }
    }
    return KAO_OK;
}

}  // namespace

extern "C" int kao_balance_disk(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width, uint16_t *rows,
                                const uint64_t *size, int32_t max_per_rack, int32_t move_leaders, uint64_t min_gain, int32_t max_rounds, int32_t dry_run,
                                int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after, uint64_t *lower_bound,
                                int32_t *status, int64_t stats[8]) {
    return balance_disk({false, false, false}, "kao_balance_disk: ",
                        {n_brokers, n_racks, rack_of, n_partitions, width, rows, size, nullptr, max_per_rack, move_leaders, min_gain, UINT64_MAX, max_rounds, dry_run,
                         n_moved, bytes_moved, peak_before, peak_after, lower_bound, status, stats});
}

extern "C" int kao_balance_disk_budget(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width, uint16_t *rows,
                                       const uint64_t *size, int32_t max_per_rack, int32_t move_leaders, uint64_t min_gain, uint64_t max_bytes,
                                       int32_t max_rounds, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before,
                                       uint64_t *peak_after, uint64_t *lower_bound, int32_t *status, int64_t stats[10]) {
    return balance_disk({true, false, false}, "kao_balance_disk_budget: ",
                        {n_brokers, n_racks, rack_of, n_partitions, width, rows, size, nullptr, max_per_rack, move_leaders, min_gain, max_bytes, max_rounds, dry_run,
                         n_moved, bytes_moved, peak_before, peak_after, lower_bound, status, stats});
}

extern "C" int kao_balance_disk_capacity(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width, uint16_t *rows,
                                         const uint64_t *size, const uint64_t *cap, int32_t max_per_rack, int32_t move_leaders, uint64_t min_gain,
                                         uint64_t max_bytes, int32_t max_rounds, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved,
                                         uint64_t peak_before[2], uint64_t peak_after[2], uint64_t lower_bound[2], int32_t *status, int64_t stats[11]) {
    const std::string fn = "kao_balance_disk_capacity: ";
    if (!cap) return fail(KAO_ERR_INVALID, fn + "null pointer");
    return balance_disk({max_bytes != UINT64_MAX, true, false}, fn,   // no budget: no grant kernel, stats[8] = stats[9] = 0
                        {n_brokers, n_racks, rack_of, n_partitions, width, rows, size, cap, max_per_rack, move_leaders, min_gain, max_bytes, max_rounds, dry_run,
                         n_moved, bytes_moved, peak_before, peak_after, lower_bound, status, stats});
}

extern "C" int kao_balance_disk_exchange(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width, uint16_t *rows,
                                         const uint64_t *size, int32_t max_per_rack, int32_t move_leaders, uint64_t min_gain, int32_t max_rounds,
                                         int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
                                         uint64_t *lower_bound, int32_t *status, int64_t stats[12]) {
    return balance_disk({false, false, true}, "kao_balance_disk_exchange: ",
                        {n_brokers, n_racks, rack_of, n_partitions, width, rows, size, nullptr, max_per_rack, move_leaders, min_gain, UINT64_MAX, max_rounds, dry_run,
                         n_moved, bytes_moved, peak_before, peak_after, lower_bound, status, stats});
}

extern "C" int kao_balance_disk_drain(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width, uint16_t *rows,
                                      const uint64_t *size, const uint8_t *drain, int32_t max_per_rack, int32_t move_leaders, uint64_t min_gain,
                                      int32_t max_rounds, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before, uint64_t *peak_after,
                                      uint64_t *lower_bound, int32_t *n_left, uint64_t *bytes_left, int32_t *status, int64_t stats[10]) {
    return balance_disk({false, false, false, true}, "kao_balance_disk_drain: ",
                        {n_brokers, n_racks, rack_of, n_partitions, width, rows, size, nullptr, max_per_rack, move_leaders, min_gain, UINT64_MAX, max_rounds, dry_run,
                         n_moved, bytes_moved, peak_before, peak_after, lower_bound, status, stats, drain, n_left, bytes_left});
}

extern "C" int kao_balance_disk_banded(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width, uint16_t *rows,
                                       const uint64_t *size, int32_t count_lo, int32_t count_hi, int32_t exchange, int32_t max_per_rack, int32_t move_leaders,
                                       uint64_t min_gain, int32_t max_rounds, int32_t dry_run, int32_t *n_moved, uint64_t *bytes_moved, uint64_t *peak_before,
                                       uint64_t *peak_after, uint64_t *lower_bound, int32_t count_range[4], int32_t *status, int64_t stats[14]) {
    DkArgs a{n_brokers, n_racks, rack_of, n_partitions, width, rows, size, nullptr, max_per_rack, move_leaders, min_gain, UINT64_MAX, max_rounds, dry_run,
             n_moved, bytes_moved, peak_before, peak_after, lower_bound, status, stats};
    a.count_lo = count_lo; a.count_hi = count_hi; a.count_range = count_range;
    return balance_disk({false, false, exchange != 0, false, true}, "kao_balance_disk_banded: ", a);
}
