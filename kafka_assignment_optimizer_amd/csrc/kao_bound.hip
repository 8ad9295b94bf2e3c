// kao_bound.hip -- K-bound: the Lagrangian dual bound "KAO-DB" of the Kafka partition-assignment model on gfx950
// (scalar replay oracle/kao_port.c::kao_port_dual_bound).
//
// lp_solve certifies optimality by branch-and-bound over the LP relaxation (README.md:135-136); here the certificate
// is the Lagrangian dual of the same 0-1 model: the coupling rows C3 (README.md:158-161), C4 (163-166) and C6 (173-176)
// are priced with integer fixed-point multipliers a[b], l[b], g[r]; the rows local to a partition (C1, C2, C5, C7) stay
// in a per-partition subproblem solved exactly (greedy follower set under the per-partition rack band + one exchange
// for the leader) by one lane over per-iteration candidate pools.  L(a,l,g) bounds the optimum from above for ANY
// multipliers, so floor(min L / kDualScale) is a valid certificate; a deflected, level-controlled Polyak subgradient
// step towards the incumbent objective drives it down.  Integer-only so that the replay agrees bit for bit.
//
// Two drivers over the same phases (pools -> subproblems -> band terms / direction -> step):
//   k_bound       one workgroup per topic, persistent over the iterations of a launch; multipliers, counters, rack
//                 tables and pools live in LDS.  Topics up to a few thousand partitions.
//   k_bound_step  one ITERATION per kernel launch, the partitions of a topic sliced over several workgroups (every
//                 workgroup rebuilds the pools -- O(B), cheap -- and solves its slice; subproblem counts meet in HBM by
//                 atomics; the LAST workgroup to finish, found by a ticket, evaluates the dual value and takes the
//                 step).  No grid barrier, no co-residency assumption: the iteration boundary is the kernel boundary.
//                 For topics of 10^4..10^5 partitions, where one compute unit per topic was what the certificate
//                 waited for.  Same arithmetic, same order of decisions: the two agree bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits.h>

#include "kao_device.h"
#include "kao_internal.h"

namespace kao {

__device__ __forceinline__ int db_sub(int m, int n, int lo, int hi) {  // element of the subdifferential closest to 0
    return m > 0 ? hi - n : (m < 0 ? lo - n : (n < lo ? lo - n : (n > hi ? hi - n : 0)));
}
// nearest multiple of 2^sh (half up; arithmetic shift)
__device__ __forceinline__ int dual_round(int v, int sh) { return ((v + (1 << (sh - 1))) >> sh) << sh; }
// Deflection d = 2^(6-k) s + floor((2^k - 1) d_prev / 2^k), a memory of about 2^k iterations: k = 2 (16 s + 3/4 d_prev) up to
// kDualDeflP partitions, k = 4 (4 s + 15/16 d_prev) beyond.  With thousands of partitions a subproblem solution is bang-bang
// (|s|^2 ~ 2e5 on the drifted 400 x 3000 topic: a price change of a thousandth flips hundreds of partitions), one subgradient
// says little, and the average over 16 of them -- the residual of an averaged, nearly LP-feasible assignment -- is a far
// better direction: that topic (LP optimum 22586) reaches 22588.8 after 4,200 iterations instead of stalling at 22601.4.
// Small topics close faster with the short memory (wide family: 174 of 175 within 1,500 iterations, 166 with k = 4).
__device__ __forceinline__ int db_defl(int n_partitions) { return n_partitions > kDualDeflP ? 4 : 2; }
__device__ __forceinline__ int db_dir(int d_prev, int s, int k) { return s * (1 << (6 - k)) + (int)(((long long)d_prev * ((1 << k) - 1)) >> k); }
// The move |step * d| carries 16 fractional bits below the multipliers' unit of the last place.  Truncating them froze
// the iterate on large topics (1000 x 30000: |d|^2 grows with the number of brokers, near the optimum every move fell below
// one unit and NO multiplier changed for 50,000 iterations): the fraction is rounded up with probability equal to itself --
// `h`, 16 bits hashed from the step number and the multiplier's index -- so the expected move is the exact one.
__device__ __forceinline__ uint32_t db_dither(uint32_t seq, uint32_t idx) {
    uint32_t h = seq * 0x9E3779B1u + idx * 0x85EBCA77u + 0x68E31DA4u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h >> 16;
}
// `step` = (gap << sh) / |d|^2 with sh in 20..40 (bound_step_length): the move is gap * 2^(6-k) d / |d|^2.
__device__ __forceinline__ int db_move(int m, long long step, int sh, int k, int d, uint32_t h) {
    const long long mag = (step * (d < 0 ? -(long long)d : (long long)d) + ((long long)h << (sh - 22 + k))) >> (sh - 6 + k);
    long long v = (long long)m - (d < 0 ? -mag : mag);
    v = v > kDualClamp ? kDualClamp : (v < -kDualClamp ? -kDualClamp : v);
    return (int)v;
}

// Wavefront arg-max of (value, lowest id): lanes hold their best (key = biased value, 0 = none; id).  Returns the lane
// that owns the winner.  `mx` receives the maximum key (0 = no lane had a candidate).
__device__ __forceinline__ int wave_argmax(uint32_t key, uint32_t id, uint32_t &mx) {
    mx = wave_umax(key);
    const unsigned long long ties = __ballot(key == mx);
    if (__popcll(ties) == 1) return (int)__builtin_ctzll(ties);
    const uint32_t sid = wave_umin(key == mx ? id : 0xFFFFFFFFu);
    return (int)__builtin_ctzll(__ballot(key == mx && id == sid));
}

// Every phase is instantiated for NE = 4 (RF and current RF <= 4: the README's range, 8 B of current assignment per partition)
// and NE = 8 (RF 5..8, round 3).  Per rack the NE best follower candidates (RF needed) and the NE + 1 best leader candidates
// (RF + 1 needed) are kept; the follower pool PF holds NE racks x NE brokers, the leader pool PL the best leader of NE + 1 racks.
template <int NE> struct BoundDims {
    static constexpr int kTF = NE, kTL = NE + 1, kPF = NE * NE, kPL = 2 * NE;
};

// wave-uniform copy of what the phases need from the topic descriptor
struct BoundTopic {
    int B, R, P, RF, rfc;
    int rep_lo, rep_hi, lead_lo, lead_hi, rack_lo, rack_hi, plo, phi;
    int w00, w01, w10, w11;   // role weights in dual fixed point
    int dk;                   // deflection memory log2 (db_defl)
};
__device__ __forceinline__ BoundTopic bound_topic(const TopicDev &T) {
    BoundTopic K;
    K.B = T.B; K.R = T.R; K.P = T.P; K.RF = T.RF; K.rfc = T.rf_cur;
    K.rep_lo = T.rep_lo; K.rep_hi = T.rep_hi; K.lead_lo = T.lead_lo; K.lead_hi = T.lead_hi;
    K.rack_lo = T.rack_lo; K.rack_hi = T.rack_hi; K.plo = T.prack_lo; K.phi = T.prack_hi;
    K.w00 = T.w00 * kDualScale; K.w01 = T.w01 * kDualScale; K.w10 = T.w10 * kDualScale; K.w11 = T.w11 * kDualScale;
    K.dk = db_defl(T.P);
    return K;
}

// LDS carve (bound_lds_bytes)
struct BoundLds {
    long long *acc;      // [2][4] : L, |s|^2, |d|^2, -
    int *ctl;            // [4]
    int *G, *DG, *NK;    // g[kRackTab], dg[kRackTab], replicas per rack in the subproblem solutions
    int *RO;             // first member of rack r in XB ([kRackTab + 2])
    int *PFb, *PFr, *PFv;  // follower pool: broker, rack, generic value [NE * NE] each
    int *PLb, *PLr, *PLv;  // best leader of the RF+1 best racks [2 * NE] each
    int *TFb, *TFv;      // per rack: kTF best followers (broker, value)
    int *TLb, *TLv;      // per rack: kTL best leaders
    int *A, *LM;         // a[maxB], l[maxB]
    int *NR, *NL;        // replicas / leaders per broker in the subproblem solutions
    uint16_t *XB;        // brokers grouped by rack (ascending inside a rack)
    uint8_t *RK;         // rack of broker
    int *DA, *DL;        // previous directions of a[], l[] (k_bound_multi only: the other drivers keep them in HBM)
    uint32_t *BW;        // broker weights bw | bwl << 16 per dense broker (launches with weighted topics), else nullptr
    uint32_t *CURP;      // current assignment, NE x u16 per partition (0xFFFF = none), when it fits next to the broker tables
};
// generic follower value F and leader value FL = F - l of broker b in rack r under the multipliers in LDS; broker weights are
// plain objective coefficients (kao_topic.broker_w on every replica, broker_wl on top for the leader)
__device__ __forceinline__ int bound_fval(const BoundLds &L, int b, int gr) {
    return -L.A[b] - gr + (L.BW ? (int)(L.BW[b] & 0xFFFFu) * kDualScale : 0);
}
__device__ __forceinline__ int bound_lval(const BoundLds &L, int b, int gr) {
    return -L.A[b] - gr - L.LM[b] + (L.BW ? (int)((L.BW[b] & 0xFFFFu) + (L.BW[b] >> 16)) * kDualScale : 0);
}
template <int NE>
__device__ __forceinline__ BoundLds bound_carve(unsigned char *smem_b, int maxB, int maxR, bool hbw, bool dirs = false) {
    using D = BoundDims<NE>;
    constexpr int kTF = D::kTF, kTL = D::kTL;
    BoundLds L;
    L.acc = reinterpret_cast<long long *>(smem_b);
    L.ctl = reinterpret_cast<int *>(smem_b + 64);
    L.G = reinterpret_cast<int *>(smem_b + 80);
    L.DG = L.G + kRackTab;
    L.NK = L.DG + kRackTab;
    L.RO = L.NK + kRackTab;
    L.PFb = L.RO + kRackTab + 2;
    L.PFr = L.PFb + D::kPF; L.PFv = L.PFr + D::kPF;
    L.PLb = L.PFv + D::kPF;
    L.PLr = L.PLb + D::kPL; L.PLv = L.PLr + D::kPL;
    L.TFb = L.PLv + D::kPL;
    L.TFv = L.TFb + maxR * kTF;
    L.TLb = L.TFv + maxR * kTF;
    L.TLv = L.TLb + maxR * kTL;
    L.A = L.TLv + maxR * kTL;
    L.LM = L.A + maxB;
    L.NR = L.LM + maxB;
    L.NL = L.NR + maxB;
    L.XB = reinterpret_cast<uint16_t *>(L.NL + maxB);
    L.RK = reinterpret_cast<uint8_t *>(L.XB + ((maxB + 7) & ~7));
    unsigned char *tail = L.RK + ((maxB + 15) & ~15);
    L.BW = hbw ? reinterpret_cast<uint32_t *>(tail) : nullptr;
    if (hbw) tail += 4 * (size_t)((maxB + 3) & ~3);
    L.DA = dirs ? reinterpret_cast<int *>(tail) : nullptr;
    L.DL = dirs ? L.DA + ((maxB + 3) & ~3) : nullptr;
    if (dirs) tail += 8 * (size_t)((maxB + 3) & ~3);
    L.CURP = reinterpret_cast<uint32_t *>(tail);
    return L;
}

template <int NE> struct CurW { uint32_t w[NE / 2]; };   // NE x u16, slot i in bits 16 (i & 1) of word i / 2
template <int NE>
__device__ __forceinline__ CurW<NE> bound_load_cur(const uint16_t *curd, int rfc, int p) {
    // NE independent loads (index clamped to the last valid slot), then masked
    const uint16_t *cur = curd + (size_t)p * rfc;
    uint32_t v[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) v[i] = cur[min(i, rfc - 1)];
    CurW<NE> c;
#pragma unroll
    for (int i = 0; i < NE / 2; ++i) c.w[i] = (2 * i < rfc ? v[2 * i] : 0xFFFFu) | ((2 * i + 1 < rfc ? v[2 * i + 1] : 0xFFFFu) << 16);
    return c;
}
template <int NE> __device__ __forceinline__ CurW<NE> bound_lds_cur(const uint32_t *curp, int p) {
    CurW<NE> c;
#pragma unroll
    for (int i = 0; i < NE / 2; ++i) c.w[i] = curp[p * (NE / 2) + i];
    return c;
}
template <int NE> __device__ __forceinline__ void bound_stage_cur(uint32_t *curp, int p, const CurW<NE> &c) {
#pragma unroll
    for (int i = 0; i < NE / 2; ++i) curp[p * (NE / 2) + i] = c.w[i];
}

// rack offsets RO (R <= 255) by thread 0, then the members of every rack from the rack-major internal index
// (x = rack * m + j; dense order kept inside a rack).  Ends with a workgroup barrier.
__device__ __forceinline__ void bound_rack_members(const BoundLds &L, const BoundPools &pl, const TopicDev &T, int tid, int nt) {
    if (tid == 0) {
        int o = 0;
        for (int r = 0; r < T.R; ++r) { L.RO[r] = o; o += pl.rsz_pool[T.rsz_off + r]; }
        L.RO[T.R] = o;
    }
    __syncthreads();
    const uint16_t *ext = pl.ext_pool + T.ext_off;
    for (int x = tid; x < T.Bx; x += nt) {
        const int r = x / T.m, jj = x - r * T.m;
        if (jj < L.RO[r + 1] - L.RO[r]) L.XB[L.RO[r] + jj] = ext[x];
    }
    __syncthreads();
}

// Phase A works on candidate pools instead of all brokers.  With values "priced weight + bonus for the partition's own
// current brokers (bonus >= 0)" and the rule "largest value, ties -> lowest broker index", the greedy pick of a round
// is always (i) one of the partition's current brokers, or (ii) one of the RF best brokers (by generic value F, then
// index) of one of the RF best racks (racks ranked by their best broker): fewer than RF picks exist before any round,
// so a better-or-equal unpicked broker of the same rack, or the best broker of a still empty better rack, would win
// otherwise.  Likewise the leader is a set member, a current broker, one of the RF+1 best brokers (by generic leader
// value FL) of a rack that holds a set member, or the best broker of one of the RF+1 best racks by FL (at least one
// of them holds no set member, and brokers of member-free racks all displace the same element).  The pools are rebuilt
// once per iteration by the workgroup; a LANE then solves a partition over <= 20 + 33 candidates, independent of B,
// with results identical to the brute-force scan of the scalar replay (oracle/kao_port.c).
//
// Phases T and R: the pools of this iteration.  Ends with a workgroup barrier.
template <int NE>
__device__ __forceinline__ void bound_pools(const BoundLds &L, const BoundTopic &K, int wave, int nw, int lane) {
    using D = BoundDims<NE>;
    constexpr int kTF = D::kTF, kTL = D::kTL;
    const int R = K.R, RF = K.RF;
    // The k-th pick of a ranking by (value descending, id ascending) is the best element strictly BEHIND the (k-1)-th in that
    // order -- ids are unique, so the order is strict and one (key, id) pair replaces the list of earlier picks.
    // ---- phase T: per rack, the kTF best followers and kTL best leaders by generic value (one wavefront per rack and ranking) ----
    for (int uu = wave; uu < 2 * R; uu += nw) {
        const int u = __builtin_amdgcn_readfirstlane(uu), r = u >> 1;
        const int x0 = L.RO[r], n = L.RO[r + 1] - x0, gr = L.G[r];
        {
            const int pass = u & 1;              // 0: followers (F), 1: leaders (FL = F - l)
            const int want = pass == 0 ? RF : RF + 1, stride = pass == 0 ? kTF : kTL;
            int *ob = pass == 0 ? L.TFb + r * kTF : L.TLb + r * kTL, *ov = pass == 0 ? L.TFv + r * kTF : L.TLv + r * kTL;
            uint32_t pk = 0xFFFFFFFFu, pb = 0;   // the previous pick (none yet: every key is below 0xFFFFFFFF -- values stay far from INT_MAX)
            for (int k = 0; k < stride; ++k) {
                int selb = -1, selv = 0;
                if (k < want && k < n) {
                    uint32_t bkey = 0, bb = 0xFFFFFFFFu;
                    for (int jj = lane; jj < n; jj += 64) {
                        const uint32_t b = L.XB[x0 + jj];
                        const int v = pass ? bound_lval(L, (int)b, gr) : bound_fval(L, (int)b, gr);
                        const uint32_t key = (uint32_t)v + 0x80000000u;
                        const bool ok = key < pk || (key == pk && b > pb);
                        if (ok && key > bkey) { bkey = key; bb = b; }   // members ascend inside a rack: the first of equal keys is the lowest id
                    }
                    uint32_t mx;
                    const int wl_ = wave_argmax(bkey, bb, mx);
                    selb = __builtin_amdgcn_readlane((int)bb, wl_);
                    selv = (int)(mx - 0x80000000u);
                    pk = mx; pb = (uint32_t)selb;
                }
                if (lane == 0) { ob[k] = selb; ov[k] = selv; }
            }
        }
    }
    __syncthreads();
    // ---- phase R: the RF best racks for followers -> pool PF (wavefront 0), the RF+1 best racks for leaders -> PL (wavefront 1) ----
    // Up to 64 racks a lane RANKS its rack against all others (independent compares instead of `want` dependent arg-max rounds:
    // phase R was a quarter of an iteration's fixed cost) and the racks of rank < want write their pool rows; beyond 64 racks the
    // arg-max rounds remain.  Same strict order (value descending, best broker's id ascending), same pools.
    if (wave < 2) {
        for (int pass = wave; pass < 2; pass += nw) {
            const int want = pass == 0 ? RF : RF + 1;
            const int *tb = pass == 0 ? L.TFb : L.TLb, *tv = pass == 0 ? L.TFv : L.TLv;
            const int stride = pass == 0 ? kTF : kTL;
            if (pass == 0) { for (int i = lane; i < D::kPF; i += 64) { L.PFb[i] = -1; L.PFr[i] = -1; L.PFv[i] = 0; } }
            else if (lane < D::kPL) { L.PLb[lane] = -1; L.PLr[lane] = -1; L.PLv[lane] = 0; }
            if (R <= 64) {
                const int myb = lane < R ? tb[lane * stride] : -1;
                const uint32_t mykey = lane < R ? (uint32_t)tv[lane * stride] + 0x80000000u : 0u;
                int rank = 0;
                for (int r2 = 0; r2 < R; ++r2) {
                    const int b2 = __builtin_amdgcn_readlane(myb, r2);
                    const uint32_t k2 = (uint32_t)__builtin_amdgcn_readlane((int)mykey, r2);
                    rank += (int)((b2 >= 0) & (k2 > mykey || (k2 == mykey && (uint32_t)b2 < (uint32_t)myb)));
                }
                if (myb >= 0 && rank < want) {
                    if (pass == 0) {
                        for (int t = 0; t < kTF; ++t) {
                            const bool have = t < RF;
                            L.PFb[rank * kTF + t] = have ? L.TFb[lane * kTF + t] : -1;
                            L.PFr[rank * kTF + t] = lane;
                            L.PFv[rank * kTF + t] = have ? L.TFv[lane * kTF + t] : 0;
                        }
                    } else { L.PLb[rank] = myb; L.PLr[rank] = lane; L.PLv[rank] = tv[lane * stride]; }
                }
            } else {
                uint32_t pk = 0xFFFFFFFFu, pb = 0;
                for (int k = 0; k < want; ++k) {
                    uint32_t bkey = 0, bid = 0xFFFFFFFFu;
                    int brk = -1;
                    for (int r = lane; r < R; r += 64) {
                        const int b = tb[r * stride];
                        const uint32_t key = (uint32_t)tv[r * stride] + 0x80000000u;
                        const bool ok = (b >= 0) & (key < pk || (key == pk && (uint32_t)b > pb));
                        if (ok && (key > bkey || (key == bkey && (uint32_t)b < bid))) { bkey = key; bid = (uint32_t)b; brk = r; }
                    }
                    if (__ballot(bkey != 0) == 0ull) break;   // nothing left: no later pick either
                    uint32_t mx;
                    const int wl_ = wave_argmax(bkey, bid, mx);
                    const int selr = __builtin_amdgcn_readlane(brk, wl_);
                    pk = mx; pb = (uint32_t)__builtin_amdgcn_readlane((int)bid, wl_);
                    if (pass == 0) {
                        if (lane < kTF) {
                            const bool have = lane < RF;
                            L.PFb[k * kTF + lane] = have ? L.TFb[selr * kTF + lane] : -1;
                            L.PFr[k * kTF + lane] = selr;
                            L.PFv[k * kTF + lane] = have ? L.TFv[selr * kTF + lane] : 0;
                        }
                    } else if (lane == 0) { L.PLb[k] = L.TLb[selr * kTL]; L.PLr[k] = selr; L.PLv[k] = L.TLv[selr * kTL]; }
                }
            }
        }
    }
    __syncthreads();
}

// Phase A: one LANE per partition of [p_begin, p_end) solves the priced subproblem over the pools; the solutions are
// counted into L.NR / L.NL / L.NK (LDS atomics), their values summed into `wsum` (per lane), `bad` = a partition without a
// solution.  kCurLds: the current assignment is staged in L.CURP (indexed by partition), otherwise read from `curd`.
template <int NE, bool kCurLds>
__device__ __forceinline__ void bound_subproblems(const BoundLds &L, const BoundTopic &K, const uint16_t *curd, int p_begin, int p_end,
                                                  int wave, int nw, int lane, long long &wsum, bool &bad) {
    using D = BoundDims<NE>;
    constexpr int kTF = D::kTF, kTL = D::kTL;
    const int B = K.B, R = K.R, RF = K.RF, plo = K.plo, phi = K.phi;
    const int w00 = K.w00, w01 = K.w01, w10 = K.w10, w11 = K.w11;
    const int *PFb = L.PFb, *PFr = L.PFr, *PFv = L.PFv, *PLb = L.PLb, *PLr = L.PLr, *PLv = L.PLv, *TLb = L.TLb, *TLv = L.TLv;
    const int *G = L.G;
    // Of a rack's ranked candidates only the first `pdepth` = min(prack_hi, RF) can enter the follower set (a later one is dominated
    // by an earlier one of the same rack, and the rack is full once `prack_hi` of them are in), and only the first pdepth + 1
    // leader candidates matter (at most pdepth of them are set members; all non-members of a rack displace the same element).
    // With the usual prack_hi = 1 that is 3 + 4 follower candidates per round instead of 12 + 4 -- same picks, same value.
    const int pdepth = min(phi, RF);
    for (int base = p_begin + wave * 64; base < p_end; base += nw * 64) {
        const int p = base + lane;
        const bool act = p < p_end;
        const CurW<NE> cw = kCurLds ? bound_lds_cur<NE>(L.CURP, min(p, p_end - 1)) : bound_load_cur<NE>(curd, K.rfc, min(p, p_end - 1));
        int cb[NE], cr[NE], cF[NE], cFL[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            cb[i] = (int)((cw.w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
            const bool v = cb[i] < B;
            const int b = v ? cb[i] : 0;
            cr[i] = L.RK[b];
            cF[i] = bound_fval(L, b, G[cr[i]]);
            cFL[i] = bound_lval(L, b, G[cr[i]]);
            if (!v) cb[i] = -1;
        }
        // objective weight of broker b in this partition: current leader / current follower / newcomer
        auto is_cur_f = [&](int b) { bool f = false;
#pragma unroll
            for (int i = 1; i < NE; ++i) f |= b == cb[i];
            return f; };
        int Gb[NE], Gf[NE], Gr[NE];
#pragma unroll
        for (int i = 0; i < NE; ++i) { Gb[i] = -1; Gf[i] = 0; Gr[i] = -1; }
        bool fail = false;
        // greedy follower set: prack_lo best of every rack first, then the best remaining under the cap; ties -> lowest b
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            if (j >= RF) break;
            const int forced = j < R * plo ? j / plo : -1;
            int bf = INT_MIN, bb = INT_MAX, br = -1;
            auto consider = [&](int b, int r, int F) {
                const int f = F + ((b == cb[0]) ? w01 : (is_cur_f(b) ? w11 : 0));
                int cnt = 0;
                bool in = false;
#pragma unroll
                for (int i = 0; i < NE - 1; ++i) { cnt += (int)(Gr[i] == r); in |= Gb[i] == b; }
                const bool ok = (b >= 0) & (forced >= 0 ? r == forced : cnt < phi) & !in;
                if (ok && (f > bf || (f == bf && b < bb))) { bf = f; bb = b; br = r; }
            };
            for (int k = 0; k < RF; ++k)
                for (int i = k * kTF; i < k * kTF + pdepth; ++i) consider(PFb[i], PFr[i], PFv[i]);
#pragma unroll
            for (int i = 0; i < NE; ++i) consider(cb[i], cr[i], cF[i]);
            if (bb == INT_MAX) { fail = true; bb = -1; bf = 0; }
            Gb[j] = bb; Gf[j] = bf; Gr[j] = br;
        }
        // leader: outside the set it displaces the cheapest element whose removal keeps the rack band
        int fG = 0;
#pragma unroll
        for (int j = 0; j < NE; ++j) fG += Gf[j];
        int cg[NE];
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            cg[j] = 0;
#pragma unroll
            for (int i = 0; i < NE; ++i) cg[j] += (int)(Gr[i] == Gr[j]);
        }
        int bv = INT_MIN, b0 = INT_MAX, be = -1, b0r = -1;
        auto lead = [&](int b, int r, int FL) {
            const int lv = FL + ((b == cb[0]) ? w00 : (is_cur_f(b) ? w10 : 0));
            int e = -1, fe = 0;
#pragma unroll
            for (int j = NE - 1; j >= 0; --j) if (Gb[j] == b) { e = j; fe = Gf[j]; }   // (a broker is in the set once)
            if (e < 0) {
                int rc = 0;
#pragma unroll
                for (int i = 0; i < NE; ++i) rc += (int)(Gr[i] == r);
                const bool full = rc >= phi;
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const bool ok = (j < RF) & (full ? Gr[j] == r : ((Gr[j] == r) | (cg[j] > plo)));
                    if (ok && (e < 0 || Gf[j] <= fe)) { e = j; fe = Gf[j]; }     // cheapest; ties -> the latest picked
                }
            }
            const int v = fG - fe + lv;
            if (b >= 0 && e >= 0 && (v > bv || (v == bv && b < b0))) { bv = v; b0 = b; be = e; b0r = r; }
        };
        if (!fail) {
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                if (j >= RF) break;
                const int b = Gb[j], r = Gr[j];
                lead(b, r, bound_lval(L, b, G[r]));                               // a set member leads
                for (int k = 0; k <= pdepth; ++k) lead(TLb[r * kTL + k], r, TLv[r * kTL + k]);   // best leaders of its rack
            }
#pragma unroll
            for (int i = 0; i < NE; ++i) lead(cb[i], cr[i], cFL[i]);              // the partition's current brokers
            for (int i = 0; i <= RF; ++i) lead(PLb[i], PLr[i], PLv[i]);           // best leader of the best racks
        }
        if (b0 == INT_MAX) fail = true;
        if (act && fail) bad = true;
        if (act && !fail) {
            wsum += bv;
#pragma unroll
            for (int j = 0; j < NE; ++j)
                if (j < RF && j != be) { atomicAdd(&L.NR[Gb[j]], 1); atomicAdd(&L.NK[Gr[j]], 1); }
            atomicAdd(&L.NR[b0], 1);
            atomicAdd(&L.NL[b0], 1);
            atomicAdd(&L.NK[b0r], 1);
        }
    }
}

// Phase B: band terms of L, subgradient s, new direction d = 16 s + floor(3 d_prev / 4); 64-bit partial sums per thread.
__device__ __forceinline__ void bound_band_terms(const BoundLds &L, const BoundTopic &K, int *g_da, int *g_dl, bool probe, int tid, int nt,
                                                 long long &cL, long long &cN, long long &cD) {
    for (int b = tid; b < K.B; b += nt) {
        const int a_ = L.A[b], l_ = L.LM[b];
        const int sa = db_sub(a_, L.NR[b], K.rep_lo, K.rep_hi), sl = db_sub(l_, L.NL[b], K.lead_lo, K.lead_hi);
        cL += (long long)a_ * (a_ > 0 ? K.rep_hi : K.rep_lo) + (long long)l_ * (l_ > 0 ? K.lead_hi : K.lead_lo);
        cN += (long long)sa * sa + (long long)sl * sl;
        if (!probe) {
            const int da = db_dir(g_da[b], sa, K.dk), dl = db_dir(g_dl[b], sl, K.dk);
            g_da[b] = da; g_dl[b] = dl;
            cD += (long long)da * da + (long long)dl * dl;
        }
    }
    if (tid < K.R) {
        const int g_ = L.G[tid], sg = db_sub(g_, L.NK[tid], K.rack_lo, K.rack_hi);
        cL += (long long)g_ * (g_ > 0 ? K.rack_hi : K.rack_lo);
        cN += (long long)sg * sg;
        if (!probe) {
            const int dg = db_dir(L.DG[tid], sg, K.dk);
            L.DG[tid] = dg;
            cD += (long long)dg * dg;
        }
    }
}

// Level control and step length of the Polyak step (every thread computes the same values).  The step aims at `level` =
// record - delta, never below the incumbent `target`; delta starts as the whole distance record -> incumbent (an incumbent
// below the optimum is an unreachable level: steps too long, the record stalls far above the optimum).  Per stage of
// kDualStage iterations the record's gain is held against delta: less than delta / 32 AND less than half a unit halves delta
// (floor 1/16), at least delta / 8 doubles it (never beyond the incumbent).  The halving test is absolute while delta is large
// and relative once delta < 16 (round 3: the purely relative test halved delta from 21 to 2.6 on the drifted 1000 x 30000
// topic with 80 units still to go -- its gain per stage is ~0.05 delta, right at the delta / 32 threshold).  The thresholds are RELATIVE because the gain per stage is itself
// proportional to delta (step length ~ delta): the first rule halved whenever a stage gained less than half a unit, which
// below delta ~ 2.5 is every stage -- delta collapsed to its floor wherever the record stood, and nothing ever widened it
// again (drifted 400 x 3000, LP optimum 22586: frozen at 22601.4 aimed at a moving incumbent; now 22586.7, a probe at 22586.5).
// The record that steers the level is the best value among the ITERATES, `bi` -- not the certificate record, which the
// rounding probes also lower: a probe value the iterate cannot reach soon reads as "no progress", and with a probe every
// 150 iterations (kao_solve's launches) the level control starved (drifted 500 x 5000: 37560.9 after 18,000 iterations in
// launches of 150, 37559.6 in launches of 2000).  `dn` is |d|^2 (already replaced by the scaled |s|^2 on a reset).
// Returns (gap << sh) / |d|^2; the shift `sh` is as large as 62 bits allow, at most 40 (with the fixed 20 bits of the first
// version the quotient was ZERO once |d|^2 > 2^32 at the smallest gap -- 1000 brokers whose counts are tens off -- and the
// iterate stopped; gap < 2^42 by K-bound's limits on P * RF * weight, so sh >= 20).
__device__ __forceinline__ long long bound_step_length(long long target, long long Lv, long long dn,
                                                       long long &lv_delta, long long &lv_rec, int &lv_since, long long &bi, int &sh) {
    long long level = target * kDualScale;
    if (lv_delta <= 0) { bi = Lv; lv_delta = bi - level; lv_rec = bi; lv_since = 0; }
    if (Lv < bi) bi = Lv;
    if (++lv_since >= kDualStage) {
        const long long prog = lv_rec - bi;
        if (prog < lv_delta / 32 && prog < kDualScale / 2) { lv_delta /= 2; if (lv_delta < kDualScale / 16) lv_delta = kDualScale / 16; }
        else if (prog >= lv_delta / 8 && bi - 2 * lv_delta >= level) lv_delta *= 2;
        lv_rec = bi; lv_since = 0;
    }
    if (bi - lv_delta > level) level = bi - lv_delta;
    long long gap = Lv - level;
    if (gap < 1) gap = 1;
    sh = min(40, max(20, __clzll(gap) - 2));
    return (gap << sh) / dn;
}

// The step along d (on a reset: along the subgradient itself), counters cleared for the next evaluation.
__device__ __forceinline__ void bound_take_step(const BoundLds &L, const BoundTopic &K, int *g_da, int *g_dl, bool reset, long long step,
                                                int sh, uint32_t seq, int tid, int nt) {
    for (int b = tid; b < K.B; b += nt) {
        int da = g_da[b], dl = g_dl[b];
        if (reset) {
            da = db_sub(L.A[b], L.NR[b], K.rep_lo, K.rep_hi) * (1 << (6 - K.dk)); dl = db_sub(L.LM[b], L.NL[b], K.lead_lo, K.lead_hi) * (1 << (6 - K.dk));
            g_da[b] = da; g_dl[b] = dl;
        }
        L.A[b] = db_move(L.A[b], step, sh, K.dk, da, db_dither(seq, (uint32_t)b));
        L.LM[b] = db_move(L.LM[b], step, sh, K.dk, dl, db_dither(seq, (uint32_t)(K.B + b)));
        L.NR[b] = 0; L.NL[b] = 0;
    }
    if (tid < K.R) {
        int dg = L.DG[tid];
        if (reset) { dg = db_sub(L.G[tid], L.NK[tid], K.rack_lo, K.rack_hi) * (1 << (6 - K.dk)); L.DG[tid] = dg; }
        L.G[tid] = db_move(L.G[tid], step, sh, K.dk, dg, db_dither(seq, (uint32_t)(2 * K.B + tid)));
        L.NK[tid] = 0;
    }
}

// search prices for K-search: the multipliers on the quarter grid (exact ties between equally priced brokers).
// export_prices 1: the record multipliers, 2: the last iterate (a, l, g point at it)
__device__ __forceinline__ void bound_export_prices(const BoundPools &pl, const TopicDev &T, const int *a, const int *l, const int *g,
                                                    const int *g_ra, const int *g_rl, const int *g_rg, int tid, int nt) {
    int *pp = pl.price_pool + T.price_off;
    const int B = T.B, R = T.R;
    const bool rec = pl.export_prices == 1;
    for (int b = tid; b < B; b += nt) {
        pp[b] = dual_round(rec ? g_ra[b] : a[b], kDualQuarterLog2);
        pp[B + b] = dual_round(rec ? g_rl[b] : l[b], kDualQuarterLog2);
    }
    for (int r = tid; r < kRackTab; r += nt) pp[2 * B + r] = r < R ? dual_round(rec ? g_rg[r] : g[r], kDualQuarterLog2) : 0;
}

// ------------------------------------------------------------------------------------------------
// k_bound_center: the exact line search along the COMMON SHIFT of every family of multipliers, once per launch (round 3)
// ------------------------------------------------------------------------------------------------
// Adding c to every multiplier of a family (replicas per broker, leaders per broker, replicas per rack) leaves every subproblem
// solution alone -- each partition pays c per replica / per leader -- so L(m + c) = const + sum_i (m_i + c) * (m_i + c > 0 ? hi : lo)
// - c * total is a convex piecewise-linear function of c alone, minimal where k = (total - n * lo) / (hi - lo) multipliers are
// positive: the (k+1)-th largest becomes 0.  Tight bands (hi == lo) do not depend on the shift.  Subgradient steps are poor at
// this one direction (its kinks sit at every multiplier's zero crossing): on slack bands -- P * RF not a multiple of the broker
// count -- the record stalled 12..20 units above the LP value (drifted 270 x 2200, LP optimum 16459: 16474.6 after 20,000
// iterations in the scalar replay; 16459 after 2,000 with the shift taken once per launch).  One workgroup per topic of the
// launch, in front of whichever driver runs it; selection by rank counting in LDS (n <= 8192, K-bound's LDS limit on brokers,
// else straight from global memory); same rule, same integers as oracle/kao_port.c::db_center (idempotent: a launch that is
// repeated by another driver finds the pivot at 0).
__device__ __forceinline__ void bound_center_family(int *g_m, int n, int lo, int hi, long long total, int *sm, int *slot, int tid, int nt) {
    if (hi <= lo || n <= 1) return;                      // uniform over the workgroup
    long long k = (total - (long long)n * lo) / (hi - lo);
    if (k < 0) k = 0;
    if (k >= n) return;
    const bool in_lds = n <= 8192;
    const int *src = g_m;
    if (in_lds) {
        for (int i = tid; i < n; i += nt) sm[i] = g_m[i];
        src = sm;
    }
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const int v = src[i];
        int gt = 0, ge = 0;
        for (int j = 0; j < n; ++j) { const int w = src[j]; gt += (int)(w > v); ge += (int)(w >= v); }
        if (gt <= k && k < ge) *slot = v;                // the element of descending rank k (every writer holds the same value)
    }
    __syncthreads();
    const long long pivot = *slot;
    for (int i = tid; i < n; i += nt) {
        long long v = (long long)src[i] - pivot;
        v = v > kDualClamp ? kDualClamp : (v < -kDualClamp ? -kDualClamp : v);
        g_m[i] = (int)v;
    }
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_bound_center(BoundPools pl) {
    __shared__ int sm[8192];
    __shared__ int slot;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int topic = pl.ids[blockIdx.x];
    const TopicDev &T = pl.topics[topic];
    const int B = T.B, R = T.R;
    int *gp = pl.dual_pool + T.dual_off;                 // a[B] l[B] da[B] dl[B] g[kRackTab] dg[kRackTab]
    const long long replicas = (long long)T.P * T.RF;
    bound_center_family(gp, B, T.rep_lo, T.rep_hi, replicas, sm, &slot, tid, nt);
    bound_center_family(gp + B, B, T.lead_lo, T.lead_hi, (long long)T.P, sm, &slot, tid, nt);
    bound_center_family(gp + 4 * B, R, T.rack_lo, T.rack_hi, replicas, sm, &slot, tid, nt);
}

// ------------------------------------------------------------------------------------------------
// k_bound: one workgroup per topic, persistent over the iterations of a launch
// ------------------------------------------------------------------------------------------------
template <int NE>
__global__ __launch_bounds__(NE == 4 ? 1024 : 512) void k_bound(BoundPools pl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
    const int topic = pl.ids[blockIdx.x];
    const TopicDev &T = pl.topics[topic];
    const BoundTopic K = bound_topic(T);
    const int B = K.B, R = K.R, P = K.P;
    const BoundLds L = bound_carve<NE>(smem_b, pl.maxB, pl.maxR, pl.bwd_pool != nullptr);
    long long *acc = L.acc;
    int *ctl = L.ctl;
    const uint8_t *rk_g = pl.rackof_pool + T.rackof_off;
    int *gp = pl.dual_pool + T.dual_off;                                // a[B] l[B] da[B] dl[B] g[kRackTab] dg[kRackTab]
    int *g_a = gp, *g_l = gp + B, *g_da = gp + 2 * B, *g_dl = gp + 3 * B, *g_g = gp + 4 * B, *g_dg = gp + 4 * B + kRackTab;
    for (int b = tid; b < B; b += nt) { L.A[b] = g_a[b]; L.LM[b] = g_l[b]; L.NR[b] = 0; L.NL[b] = 0; L.RK[b] = rk_g[b]; }
    if (L.BW) for (int b = tid; b < B; b += nt) L.BW[b] = T.has_bw ? pl.bwd_pool[T.bwd_off + b] : 0u;
    for (int r = tid; r < kRackTab; r += nt) { L.G[r] = r < R ? g_g[r] : 0; L.DG[r] = r < R ? g_dg[r] : 0; L.NK[r] = 0; }
    if (tid < 8) acc[tid] = 0;
    if (tid < 4) ctl[tid] = 0;
    const uint16_t *curd = pl.curd_pool + T.curd_off;
    if (pl.cur_in_lds)
        for (int p = tid; p < P; p += nt) bound_stage_cur<NE>(L.CURP, p, bound_load_cur<NE>(curd, K.rfc, p));
    bound_rack_members(L, pl, T, tid, nt);
    long long best = pl.best_L[topic];
    const long long target = pl.target[topic];
    // level control (every thread keeps the same copy): distance record -> level, record at stage start, iterations in stage
    long long *g_lv = reinterpret_cast<long long *>(gp + 4 * B + 2 * kRackTab);
    // the multipliers of the record (smallest) dual value: what the search prices are taken from
    int *g_ra = gp + 4 * B + 2 * kRackTab + 8, *g_rl = g_ra + B, *g_rg = g_rl + B;
    long long lv_delta = g_lv[0], lv_rec = g_lv[1];
    // g_lv[2] = iterations in the stage | steps taken so far (over all launches: the dither sequence number) << 8
    int lv_since = (int)(g_lv[2] & 0xFF);
    uint32_t lv_seq = (uint32_t)(g_lv[2] >> 8);
    long long lv_bi = g_lv[3];               // best dual value among the iterates (the probes do not count)
    int flags = 0, it = 0;
    // After the last iteration of a launch the dual function is also PROBED at the multipliers rounded to the quarter and to
    // the half grid (optimal multipliers of this model tend to be small fractions: a subgradient iterate hovers a few
    // thousandths around them, the rounded point hits them exactly -- drifted 100 x 1000 topic: iterate 7430.6, rounded 7430.0
    // = the LP optimum).  A probe evaluates L only: no direction update, no step; the iterate is restored afterwards.
    const int n_steps = pl.iters + kDualProbes;
    for (int stp = 0; stp < n_steps; ++stp) {
        const int par = stp & 1;
        const bool probe = stp >= pl.iters;
        if (probe) {
            if (stp == pl.iters) {  // park the iterate in HBM (the epilogue writes the same values again)
                for (int b = tid; b < B; b += nt) { g_a[b] = L.A[b]; g_l[b] = L.LM[b]; }
                if (tid < R) g_g[tid] = L.G[tid];
            }
            const int sh = stp == pl.iters ? kDualQuarterLog2 : kDualQuarterLog2 + 1;
            for (int b = tid; b < B; b += nt) { L.A[b] = dual_round(g_a[b], sh); L.LM[b] = dual_round(g_l[b], sh); }
            if (tid < R) L.G[tid] = dual_round(g_g[tid], sh);
            __syncthreads();
        }
        bound_pools<NE>(L, K, wave, nw, lane);
        long long wsum = 0;
        bool bad = false;
        if (pl.cur_in_lds) bound_subproblems<NE, true>(L, K, curd, 0, P, wave, nw, lane, wsum, bad);
        else bound_subproblems<NE, false>(L, K, curd, 0, P, wave, nw, lane, wsum, bad);
        bad = __ballot(bad) != 0ull;
        wsum = wave_sum64(wsum);
        if (lane == 0) {
            if (wsum) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[par * 4 + 0]), (unsigned long long)wsum);
            if (bad) atomicOr(&ctl[0], 4);
        }
        __syncthreads();
        if (ctl[0] & 4) { if (!probe) flags |= 4; break; }
        long long cL = 0, cN = 0, cD = 0;
        bound_band_terms(L, K, g_da, g_dl, probe, tid, nt, cL, cN, cD);
        const bool owns = wave * 64 < max(B, R);  // wavefronts without a broker or rack skip the 64-bit reductions
        if (owns) { cL = wave_sum64(cL); cN = wave_sum64(cN); cD = wave_sum64(cD); }
        if (lane == 0 && owns) {
            if (cL) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[par * 4 + 0]), (unsigned long long)cL);
            if (cN) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[par * 4 + 1]), (unsigned long long)cN);
            if (cD) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[par * 4 + 2]), (unsigned long long)cD);
        }
        __syncthreads();
        // ---- phase C: stop tests, Polyak step along d, reset the counters ----
        const long long Lv = acc[par * 4 + 0], nrm = acc[par * 4 + 1];
        long long dn = acc[par * 4 + 2];
        if (Lv < best) {  // a new record (same decision in every thread): keep its multipliers
            best = Lv;
            for (int b = tid; b < B; b += nt) { g_ra[b] = L.A[b]; g_rl[b] = L.LM[b]; }
            if (tid < R) g_rg[tid] = L.G[tid];
        }
        if (probe) {  // a probe only records the value; back to the iterate, counters cleared for the next evaluation
            for (int b = tid; b < B; b += nt) { L.A[b] = g_a[b]; L.LM[b] = g_l[b]; L.NR[b] = 0; L.NL[b] = 0; }
            if (tid < R) { L.G[tid] = g_g[tid]; L.NK[tid] = 0; }
            if (tid < 4) acc[(par ^ 1) * 4 + tid] = 0;
            if (best < (target + 1) * kDualScale) flags |= 1;
            __syncthreads();
            continue;
        }
        ++it;
        if (best < (target + 1) * kDualScale) { flags |= 1; break; }
        if (nrm == 0) { flags |= 2; break; }
        const bool reset = dn == 0;  // the memory cancelled the subgradient: restart from it
        if (reset) dn = nrm << (2 * (6 - K.dk));
        int sh;
        const long long step = bound_step_length(target, Lv, dn, lv_delta, lv_rec, lv_since, lv_bi, sh);
        bound_take_step(L, K, g_da, g_dl, reset, step, sh, lv_seq++, tid, nt);
        if (tid < 4) acc[(par ^ 1) * 4 + tid] = 0;
        __syncthreads();
    }
    // ---- epilogue: multipliers and the best dual value go back to HBM for the next launch ----
    for (int b = tid; b < B; b += nt) { g_a[b] = L.A[b]; g_l[b] = L.LM[b]; }
    if (tid < R) { g_g[tid] = L.G[tid]; g_dg[tid] = L.DG[tid]; }
    if (pl.export_prices) bound_export_prices(pl, T, L.A, L.LM, L.G, g_ra, g_rl, g_rg, tid, nt);  // own stores or an earlier launch's
    if (tid == 0) {
        g_lv[0] = lv_delta; g_lv[1] = lv_rec; g_lv[2] = (long long)lv_since | ((long long)lv_seq << 8); g_lv[3] = lv_bi;
        pl.best_L[topic] = best;
        pl.info[topic * 4 + 0] += it;
        pl.info[topic * 4 + 1] = flags;
    }
}

// ------------------------------------------------------------------------------------------------
// k_bound_step: ONE iteration (or probe) per launch, a topic's partitions sliced over several workgroups
// ------------------------------------------------------------------------------------------------
// Per-topic control block in HBM (BoundWide::ctl, 16 x int64; the second half belongs to k_bound_multi): [0] sum of the subproblem values of this step, then as
// int32 from byte 8: [2] ticket, [3] bad, [4] stop (a launch sequence ended: later steps of the sequence return at once).
// Counters cnt_pool + TopicDev::cnt_off: NR[B] NL[B] NK[kRackTab], all zero between steps (the last workgroup clears them).
__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(64) void k_bound_begin(BoundPools pl, BoundWide wd, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int topic = pl.ids[i];
    pl.info[topic * 4 + 1] = 0;
    reinterpret_cast<int *>(wd.ctl + (size_t)topic * 16)[4] = 0;
}

// mode 0: iteration; 1 / 2: probe at the multipliers rounded to the quarter / half grid
template <int NE>
__global__ __launch_bounds__(NE == 4 ? 1024 : 512) void k_bound_step(BoundPools pl, BoundWide wd, int mode) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
    const int2 bm = wd.map[blockIdx.x];
    const int topic = bm.x, slice = bm.y;
    long long *gctl = wd.ctl + (size_t)topic * 16;
    int *gci = reinterpret_cast<int *>(gctl);
    if (gci[4]) return;   // written by an earlier launch only: the same answer in every workgroup of the topic
    const TopicDev &T = pl.topics[topic];
    const BoundTopic K = bound_topic(T);
    const int B = K.B, R = K.R, P = K.P;
    const bool probe = mode != 0;
    const BoundLds L = bound_carve<NE>(smem_b, pl.maxB, pl.maxR, pl.bwd_pool != nullptr);
    const uint8_t *rk_g = pl.rackof_pool + T.rackof_off;
    int *gp = pl.dual_pool + T.dual_off;
    int *g_a = gp, *g_l = gp + B, *g_da = gp + 2 * B, *g_dl = gp + 3 * B, *g_g = gp + 4 * B, *g_dg = gp + 4 * B + kRackTab;
    const int rsh = mode == 1 ? kDualQuarterLog2 : kDualQuarterLog2 + 1;
    for (int b = tid; b < B; b += nt) {
        const int a_ = g_a[b], l_ = g_l[b];
        L.A[b] = probe ? dual_round(a_, rsh) : a_; L.LM[b] = probe ? dual_round(l_, rsh) : l_;
        L.NR[b] = 0; L.NL[b] = 0; L.RK[b] = rk_g[b];
        if (L.BW) L.BW[b] = T.has_bw ? pl.bwd_pool[T.bwd_off + b] : 0u;
    }
    for (int r = tid; r < kRackTab; r += nt) {
        const int g_ = r < R ? g_g[r] : 0;
        L.G[r] = probe ? dual_round(g_, rsh) : g_; L.DG[r] = r < R ? g_dg[r] : 0; L.NK[r] = 0;
    }
    if (tid < 8) L.acc[tid] = 0;
    bound_rack_members(L, pl, T, tid, nt);
    bound_pools<NE>(L, K, wave, nw, lane);
    // ---- this workgroup's slice of the subproblems ----
    const int p_begin = slice * wd.chunk, p_end = min(P, p_begin + wd.chunk);
    const int n_slices = (P + wd.chunk - 1) / wd.chunk;
    long long wsum = 0;
    bool bad = false;
    // (a slice's upper end clamps the loads of its idle lanes, as P does in k_bound: the values are never used)
    bound_subproblems<NE, false>(L, K, pl.curd_pool + T.curd_off, p_begin, p_end, wave, nw, lane, wsum, bad);
    bad = __ballot(bad) != 0ull;
    wsum = wave_sum64(wsum);
    if (lane == 0) {
        if (wsum) atomicAdd(reinterpret_cast<unsigned long long *>(&L.acc[0]), (unsigned long long)wsum);
        if (bad) atomicOr(&gci[3], 1);
    }
    __syncthreads();
    int *cnt = wd.cnt_pool + T.cnt_off;   // NR[B] NL[B] NK[kRackTab]
    if (n_slices > 1) {
        for (int b = tid; b < B; b += nt) {
            const int nr = L.NR[b], nl = L.NL[b];
            if (nr) atomicAdd(&cnt[b], nr);
            if (nl) atomicAdd(&cnt[B + b], nl);
        }
        if (tid < R) { const int nk = L.NK[tid]; if (nk) atomicAdd(&cnt[2 * B + tid], nk); }
        if (tid == 0 && L.acc[0]) atomicAdd(reinterpret_cast<unsigned long long *>(&gctl[0]), (unsigned long long)L.acc[0]);
        __threadfence();
        __syncthreads();
        if (tid == 0) s_last = atomicAdd(&gci[2], 1) == n_slices - 1;
        __syncthreads();
        if (!s_last) return;
        // ---- the last workgroup of the topic: totals in, counters cleared for the next step ----
        __threadfence();
        for (int b = tid; b < B; b += nt) {
            L.NR[b] = ld_agent(&cnt[b]); L.NL[b] = ld_agent(&cnt[B + b]);
            cnt[b] = 0; cnt[B + b] = 0;
        }
        if (tid < R) { L.NK[tid] = ld_agent(&cnt[2 * B + tid]); cnt[2 * B + tid] = 0; }
        if (tid == 0) {
            L.acc[0] = __hip_atomic_load(&gctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            gctl[0] = 0; gci[2] = 0;
        }
        __syncthreads();
    }
    const int any_bad = ld_agent(&gci[3]);
    __syncthreads();
    if (tid == 0 && any_bad) gci[3] = 0;
    if (any_bad) {   // a partition without a subproblem solution: no bound from this topic
        if (tid == 0) { if (!probe) pl.info[topic * 4 + 1] |= 4; gci[4] = 1; }
        return;
    }
    long long cL = 0, cN = 0, cD = 0;
    bound_band_terms(L, K, g_da, g_dl, probe, tid, nt, cL, cN, cD);
    if (!probe && tid < R) g_dg[tid] = L.DG[tid];   // the directions persist even when the sequence ends in this step
    const bool owns = wave * 64 < max(B, R);
    if (owns) { cL = wave_sum64(cL); cN = wave_sum64(cN); cD = wave_sum64(cD); }
    if (lane == 0 && owns) {
        if (cL) atomicAdd(reinterpret_cast<unsigned long long *>(&L.acc[0]), (unsigned long long)cL);
        if (cN) atomicAdd(reinterpret_cast<unsigned long long *>(&L.acc[1]), (unsigned long long)cN);
        if (cD) atomicAdd(reinterpret_cast<unsigned long long *>(&L.acc[2]), (unsigned long long)cD);
    }
    __syncthreads();
    // ---- phase C ----
    long long *g_lv = reinterpret_cast<long long *>(gp + 4 * B + 2 * kRackTab);
    int *g_ra = gp + 4 * B + 2 * kRackTab + 8, *g_rl = g_ra + B, *g_rg = g_rl + B;
    const long long Lv = L.acc[0], nrm = L.acc[1];
    long long dn = L.acc[2];
    long long best = pl.best_L[topic];
    const long long target = pl.target[topic];
    long long lv_delta = g_lv[0], lv_rec = g_lv[1];
    int lv_since = (int)(g_lv[2] & 0xFF);
    const uint32_t lv_seq = (uint32_t)(g_lv[2] >> 8);
    long long lv_bi = g_lv[3];
    __syncthreads();   // every thread holds the state of the previous step before thread 0 rewrites it
    if (Lv < best) {
        best = Lv;
        for (int b = tid; b < B; b += nt) { g_ra[b] = L.A[b]; g_rl[b] = L.LM[b]; }
        if (tid < R) g_rg[tid] = L.G[tid];
        if (tid == 0) pl.best_L[topic] = best;
    }
    const bool reached = best < (target + 1) * kDualScale;
    if (probe) {
        if (tid == 0 && reached) pl.info[topic * 4 + 1] |= 1;
        return;
    }
    if (tid == 0) pl.info[topic * 4 + 0] += 1;
    if (reached || nrm == 0) {
        if (tid == 0) { pl.info[topic * 4 + 1] |= reached ? 1 : 2; gci[4] = 1; }
        return;
    }
    const bool reset = dn == 0;
    if (reset) dn = nrm << (2 * (6 - K.dk));
    int sh;
    const long long step = bound_step_length(target, Lv, dn, lv_delta, lv_rec, lv_since, lv_bi, sh);
    bound_take_step(L, K, g_da, g_dl, reset, step, sh, lv_seq, tid, nt);
    for (int b = tid; b < B; b += nt) { g_a[b] = L.A[b]; g_l[b] = L.LM[b]; }
    if (tid < R) { g_g[tid] = L.G[tid]; g_dg[tid] = L.DG[tid]; }
    if (tid == 0) { g_lv[0] = lv_delta; g_lv[1] = lv_rec; g_lv[2] = (long long)lv_since | (((long long)lv_seq + 1) << 8); g_lv[3] = lv_bi; }
}

// ------------------------------------------------------------------------------------------------
// k_bound_multi: PERSISTENT over the iterations of a launch like k_bound, a topic's partitions sliced over several workgroups
// like k_bound_step (round 3; VERDICT r02 item 4: k_bound_step spent 33..47 us per iteration on a kernel boundary, an HBM round
// trip of the multipliers and a ticket -- and a 2,000-partition topic 52 us in the one workgroup of k_bound).
// Every workgroup of a topic keeps the WHOLE dual state in LDS (multipliers, directions, level control) and takes every step
// itself -- redundantly, in integers, so all copies stay identical; only the subproblem counts of its slice leave the workgroup:
// they are added into one of three rotating count buffers in HBM, the topic's workgroups meet at a barrier (a monotonic counter
// in HBM), and everyone reads the totals back.  One barrier per iteration; buffer (i-1) mod 3 is cleared after barrier i (all
// its readers have arrived at barrier i, its next writers are behind barrier i+1).  Slice 0 owns the state in HBM: the record
// multipliers and the iterate parked before the probes go to a SHADOW area and are committed after the last barrier, so a
// launch that gives up commits nothing.  Giving up: a workgroup that waits longer than kMultiPatience at a barrier raises the
// topic's abort flag (the topic's workgroups are not all resident -- other persistent kernels hold the compute units); everyone
// leaves, flag 16 is reported, and the host repeats the launch with k_bound_step and stops using this driver for the session.
// Same arithmetic, same order of decisions as the other two drivers: the replay tests hold bit for bit.
// Control block (BoundWide::ctl + topic * 16 + 8, 8 x int64): [0..2] value sums of the three buffers; as int32 from byte 24:
// [0] barrier counter | abort mark (bit 30), [1] unused, [2..4] "a partition had no solution" per buffer.
constexpr long long kMultiPatience = 30000000;   // ticks of the 100 MHz constant clock: 0.3 s
constexpr int kMultiAbortBit = 1 << 30;           // in the barrier counter (arrivals stay far below: iterations x slices)
__device__ __forceinline__ void st_agent(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// zeroes what a launch of k_bound_multi (or a sequence of k_bound_step) expects to be zero: one workgroup per topic
__global__ __launch_bounds__(256) void k_bound_multi_begin(BoundPools pl, BoundWide wd) {
    const int topic = pl.ids[blockIdx.x];
    const TopicDev &T = pl.topics[topic];
    int *cnt = wd.cnt_pool + T.cnt_off;
    const int n = 3 * (2 * T.B + kRackTab);
    for (int i = threadIdx.x; i < n; i += blockDim.x) cnt[i] = 0;
    long long *ctl = wd.ctl + (size_t)topic * 16;
    if (threadIdx.x < 16) ctl[threadIdx.x] = 0;
    if (threadIdx.x == 0) pl.info[topic * 4 + 1] = 0;
}

template <int NE>
__global__ __launch_bounds__(NE == 4 ? 1024 : 512) void k_bound_multi(BoundPools pl, BoundWide wd) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    __shared__ int s_go, s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
    const int2 bm = wd.map[blockIdx.x];
    const int topic = bm.x, slice = bm.y;
    const TopicDev &T = pl.topics[topic];
    const BoundTopic K = bound_topic(T);
    const int B = K.B, R = K.R, P = K.P;
    BoundLds L = bound_carve<NE>(smem_b, pl.maxB, pl.maxR, pl.bwd_pool != nullptr, true);
    long long *acc = L.acc;
    long long *msum = wd.ctl + (size_t)topic * 16 + 8;
    int *mi = reinterpret_cast<int *>(msum + 3);   // [0] barrier | abort mark, [2..4] bad
    const int n_slices = (P + wd.chunk - 1) / wd.chunk;
    const int p_begin = slice * wd.chunk, p_end = min(P, p_begin + wd.chunk);
    const bool owner = slice == 0;
    int *gp = pl.dual_pool + T.dual_off;
    int *g_a = gp, *g_l = gp + B, *g_da = gp + 2 * B, *g_dl = gp + 3 * B, *g_g = gp + 4 * B, *g_dg = gp + 4 * B + kRackTab;
    long long *g_lv = reinterpret_cast<long long *>(gp + 4 * B + 2 * kRackTab);
    int *g_ra = gp + 4 * B + 2 * kRackTab + 8, *g_rl = g_ra + B, *g_rg = g_rl + B;
    const int cstride = 2 * B + kRackTab;
    int *cnt0 = wd.cnt_pool + T.cnt_off;            // three count buffers NR[B] NL[B] NK[kRackTab], then the shadow area
    int *sh_a = cnt0 + 3 * cstride, *sh_l = sh_a + B, *sh_g = sh_l + B, *sh_ra = sh_g + kRackTab, *sh_rl = sh_ra + B, *sh_rg = sh_rl + B;
    const uint8_t *rk_g = pl.rackof_pool + T.rackof_off;
    for (int b = tid; b < B; b += nt) {
        L.A[b] = g_a[b]; L.LM[b] = g_l[b]; L.DA[b] = g_da[b]; L.DL[b] = g_dl[b]; L.NR[b] = 0; L.NL[b] = 0; L.RK[b] = rk_g[b];
        if (L.BW) L.BW[b] = T.has_bw ? pl.bwd_pool[T.bwd_off + b] : 0u;
    }
    for (int r = tid; r < kRackTab; r += nt) { L.G[r] = r < R ? g_g[r] : 0; L.DG[r] = r < R ? g_dg[r] : 0; L.NK[r] = 0; }
    if (tid < 8) acc[tid] = 0;
    {   // this slice's current assignment stays in LDS for the whole launch (indexed by the absolute partition number)
        const uint16_t *curd = pl.curd_pool + T.curd_off;
        L.CURP -= (size_t)p_begin * (NE / 2);
        for (int p = p_begin + tid; p < p_end; p += nt) bound_stage_cur<NE>(L.CURP, p, bound_load_cur<NE>(curd, K.rfc, p));
    }
    bound_rack_members(L, pl, T, tid, nt);
    long long best = pl.best_L[topic];
    const long long target = pl.target[topic];
    long long lv_delta = g_lv[0], lv_rec = g_lv[1];
    int lv_since = (int)(g_lv[2] & 0xFF);
    uint32_t lv_seq = (uint32_t)(g_lv[2] >> 8);
    long long lv_bi = g_lv[3];
    int flags = 0, it = 0, arrivals = 0;
    bool rec = false, parked = false, aborted = false;
    const int n_steps = pl.iters + kDualProbes;
#ifdef KAO_BOUND_PROFILE   // where an iteration's time goes (slice 0, thread 0; 100 MHz ticks per phase, printed at the end)
    long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt0 = (long long)wall_clock64();
#define KAO_PROF_MARK(i) { const long long pt1 = (long long)wall_clock64(); prof[i] += pt1 - pt0; pt0 = pt1; }
#else
#define KAO_PROF_MARK(i)
#endif
    for (int stp = 0; stp < n_steps; ++stp) {
        const int buf = stp % 3;
        const bool probe = stp >= pl.iters;
        if (probe) {
            if (stp == pl.iters) {   // the iterate, parked for the commit (the probes round it in place)
                if (owner) {
                    for (int b = tid; b < B; b += nt) { sh_a[b] = L.A[b]; sh_l[b] = L.LM[b]; }
                    if (tid < R) sh_g[tid] = L.G[tid];
                }
                parked = true;
            }
            // probe 1 rounds the iterate (still in LDS) to the quarter grid; probe 2 rounds the PARKED iterate to the half grid: slice 0
            // wrote it before it arrived at probe 1's barrier, which every workgroup has left by now
            __syncthreads();
            if (stp == pl.iters) {
                for (int b = tid; b < B; b += nt) { L.A[b] = dual_round(L.A[b], kDualQuarterLog2); L.LM[b] = dual_round(L.LM[b], kDualQuarterLog2); }
                if (tid < R) L.G[tid] = dual_round(L.G[tid], kDualQuarterLog2);
            } else {
                for (int b = tid; b < B; b += nt) {
                    L.A[b] = dual_round(ld_agent(&sh_a[b]), kDualQuarterLog2 + 1); L.LM[b] = dual_round(ld_agent(&sh_l[b]), kDualQuarterLog2 + 1);
                }
                if (tid < R) L.G[tid] = dual_round(ld_agent(&sh_g[tid]), kDualQuarterLog2 + 1);
            }
            __syncthreads();
        }
        KAO_PROF_MARK(5)
        bound_pools<NE>(L, K, wave, nw, lane);
        KAO_PROF_MARK(0)
        long long wsum = 0;
        bool bad = false;
        bound_subproblems<NE, true>(L, K, nullptr, p_begin, p_end, wave, nw, lane, wsum, bad);
        bad = __ballot(bad) != 0ull;
        wsum = wave_sum64(wsum);
        if (tid == 0) s_bad = 0;
        __syncthreads();
        if (lane == 0) {
            if (wsum) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[0]), (unsigned long long)wsum);
            if (bad) { atomicOr(&s_bad, 1); if (n_slices > 1) atomicOr(&mi[2 + buf], 1); }
        }
        __syncthreads();
        KAO_PROF_MARK(1)
        int *cnt = cnt0 + buf * cstride;
        // (replicas | leaders << 32 of a broker travel as ONE 64-bit atomic: the HBM atomics of ~60 workgroups on the same 2 B
        //  addresses are what publish + barrier cost at 1000 brokers x 30,000 partitions -- 17 of 42 us before the packing)
        unsigned long long *c64 = reinterpret_cast<unsigned long long *>(cnt);
        if (n_slices > 1) {
            for (int b = tid; b < B; b += nt) {
                const unsigned long long v = (unsigned long long)(uint32_t)L.NR[b] | ((unsigned long long)(uint32_t)L.NL[b] << 32);
                if (v) atomicAdd(&c64[b], v);
            }
            if (tid < R) { const int nk = L.NK[tid]; if (nk) atomicAdd(&cnt[2 * B + tid], nk); }
            if (tid == 0 && acc[0]) atomicAdd(reinterpret_cast<unsigned long long *>(&msum[buf]), (unsigned long long)acc[0]);
            __threadfence();
            __syncthreads();
            KAO_PROF_MARK(2)
            // ---- the barrier of this evaluation ----
            ++arrivals;
            if (tid == 0) {
                atomicAdd(&mi[0], 1);
                const int goal = arrivals * n_slices;
                const long long t0 = wall_clock64();
                // Arrivals and the abort mark live in ONE word, and the mark is set by compare-and-swap on a value that is still
                // short of the goal: either every workgroup of the topic sees the mark at this barrier (nobody commits, flag 16) or
                // the mark is never set (with a separate flag a slice could pass the last barrier and commit while
                // another timed out, and the host's repeat then ran that topic's iterations twice).
                int go = 1;
                for (;;) {
                    const int v = ld_agent(&mi[0]);
                    if (v & kMultiAbortBit) { go = 0; break; }
                    if (v >= goal) break;
                    __builtin_amdgcn_s_sleep(1);
                    if ((long long)wall_clock64() - t0 > kMultiPatience && atomicCAS(&mi[0], v, v | kMultiAbortBit) == v) { go = 0; break; }
                }
                __threadfence();
                s_go = go;
            }
            __syncthreads();
            KAO_PROF_MARK(3)
            if (!s_go) { aborted = true; break; }
            // totals in; the buffer of the previous evaluation is cleared (its readers have all passed through this barrier)
            for (int b = tid; b < B; b += nt) {
                const unsigned long long v = __hip_atomic_load(&c64[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                L.NR[b] = (int)(uint32_t)v; L.NL[b] = (int)(uint32_t)(v >> 32);
            }
            if (tid < R) L.NK[tid] = ld_agent(&cnt[2 * B + tid]);
            if (tid == 0) acc[0] = __hip_atomic_load(&msum[buf], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tid == nt - 1) s_bad = ld_agent(&mi[2 + buf]);
            if (stp > 0) {
                const int pb = (stp - 1) % 3;
                int *pc = cnt0 + pb * cstride;
                for (int i = slice * nt + tid; i < cstride; i += n_slices * nt) st_agent(&pc[i], 0);
                if (owner && tid == 0) {
                    __hip_atomic_store(&msum[pb], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    st_agent(&mi[2 + pb], 0);
                }
            }
            __syncthreads();
            KAO_PROF_MARK(4)
        }
        if (s_bad) { if (!probe) flags |= 4; break; }
        long long cL = 0, cN = 0, cD = 0;
        bound_band_terms(L, K, L.DA, L.DL, probe, tid, nt, cL, cN, cD);
        const bool owns = wave * 64 < max(B, R);
        if (owns) { cL = wave_sum64(cL); cN = wave_sum64(cN); cD = wave_sum64(cD); }
        if (lane == 0 && owns) {
            if (cL) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[0]), (unsigned long long)cL);
            if (cN) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[1]), (unsigned long long)cN);
            if (cD) atomicAdd(reinterpret_cast<unsigned long long *>(&acc[2]), (unsigned long long)cD);
        }
        __syncthreads();
        KAO_PROF_MARK(6)
        // ---- phase C (every workgroup of the topic takes the same decisions) ----
        const long long Lv = acc[0], nrm = acc[1];
        long long dn = acc[2];
        __syncthreads();
        if (tid < 4) acc[tid] = 0;
        if (Lv < best) {
            best = Lv;
            rec = true;
            if (owner) {
                for (int b = tid; b < B; b += nt) { sh_ra[b] = L.A[b]; sh_rl[b] = L.LM[b]; }
                if (tid < R) sh_rg[tid] = L.G[tid];
            }
        }
        if (probe) {
            if (best < (target + 1) * kDualScale) flags |= 1;
            for (int b = tid; b < B; b += nt) { L.NR[b] = 0; L.NL[b] = 0; }
            if (tid < R) L.NK[tid] = 0;
            __syncthreads();
            continue;
        }
        ++it;
        if (best < (target + 1) * kDualScale) { flags |= 1; break; }
        if (nrm == 0) { flags |= 2; break; }
        const bool reset = dn == 0;
        if (reset) dn = nrm << (2 * (6 - K.dk));
        int sh;
        const long long step = bound_step_length(target, Lv, dn, lv_delta, lv_rec, lv_since, lv_bi, sh);
        bound_take_step(L, K, L.DA, L.DL, reset, step, sh, lv_seq++, tid, nt);
        __syncthreads();
    }
#ifdef KAO_BOUND_PROFILE
    if (owner && tid == 0)
        printf("[k_bound_multi] topic %d P %d B %d slices %d it %d: pools %lld subproblems %lld publish %lld barrier %lld totals %lld band terms %lld step %lld (x 10 ns)\n",
               topic, P, B, n_slices, it, prof[0], prof[1], prof[2], prof[3], prof[4], prof[6], prof[5]);
#endif
    if (aborted) {
        if (tid == 0) atomicOr(&pl.info[topic * 4 + 1], 16);
        return;
    }
    // ---- commit (slice 0): a stop inside the iterations leaves the iterate in LDS, the probes left it parked in the shadow ----
    if (!owner) return;
    __syncthreads();
    if (parked) {
        for (int b = tid; b < B; b += nt) { g_a[b] = sh_a[b]; g_l[b] = sh_l[b]; }
        if (tid < R) g_g[tid] = sh_g[tid];
    } else {
        for (int b = tid; b < B; b += nt) { g_a[b] = L.A[b]; g_l[b] = L.LM[b]; }
        if (tid < R) g_g[tid] = L.G[tid];
    }
    for (int b = tid; b < B; b += nt) { g_da[b] = L.DA[b]; g_dl[b] = L.DL[b]; }
    if (tid < R) g_dg[tid] = L.DG[tid];
    if (rec) {
        for (int b = tid; b < B; b += nt) { g_ra[b] = sh_ra[b]; g_rl[b] = sh_rl[b]; }
        if (tid < R) g_rg[tid] = sh_rg[tid];
    }
    if (tid == 0) {
        g_lv[0] = lv_delta; g_lv[1] = lv_rec; g_lv[2] = (long long)lv_since | ((long long)lv_seq << 8); g_lv[3] = lv_bi;
        pl.best_L[topic] = best;
        pl.info[topic * 4 + 0] += it;
        atomicOr(&pl.info[topic * 4 + 1], flags);
    }
}

// end of a launch sequence: the search prices (k_bound's epilogue)
__global__ __launch_bounds__(256) void k_bound_finish(BoundPools pl) {
    const int topic = pl.ids[blockIdx.x];
    const TopicDev &T = pl.topics[topic];
    const int B = T.B;
    const int *gp = pl.dual_pool + T.dual_off;
    const int *g_ra = gp + 4 * B + 2 * kRackTab + 8, *g_rl = g_ra + B, *g_rg = g_rl + B;
    if (pl.export_prices) bound_export_prices(pl, T, gp, gp + B, gp + 4 * B, g_ra, g_rl, g_rg, threadIdx.x, blockDim.x);
}

// ------------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------------
size_t bound_lds_bytes(int maxB, int maxP, int maxR, bool cur_in_lds, int ne, bool hbw, bool dirs) {
    const size_t pf = (size_t)ne * ne, pl = 2 * (size_t)ne, tf = (size_t)ne, tl = (size_t)ne + 1;
    size_t n = 80 + (3 * (size_t)kRackTab + kRackTab + 2 + 3 * pf + 3 * pl) * 4 + (size_t)maxR * (2 * tf + 2 * tl) * 4;
    n += 16 * (size_t)maxB + 2 * (((size_t)maxB + 7) & ~(size_t)7) + (((size_t)maxB + 15) & ~(size_t)15);
    if (hbw) n += 4 * (((size_t)maxB + 3) & ~(size_t)3);
    if (dirs) n += 8 * (((size_t)maxB + 3) & ~(size_t)3);
    n = (n + 7) & ~(size_t)7;
    return n + (cur_in_lds ? 2 * (size_t)ne * (size_t)maxP : 0);
}

static int g_attr_bound_dev[kAttrDevices][2] = {{0}}, g_attr_step_dev[kAttrDevices][2] = {{0}};

void launch_bound_center(const BoundPools &pools, int n_topics, void *stream) {
    if (pools.iters > 0) hipLaunchKernelGGL(k_bound_center, dim3(n_topics), dim3(256), 0, static_cast<hipStream_t>(stream), pools);
}

void launch_bound(const BoundPools &pools, int n_blocks, int waves, void *stream) {
    const bool ne8 = pools.ne == 8;
    const size_t lds = bound_lds_bytes(pools.maxB, pools.maxP, pools.maxR, pools.cur_in_lds != 0, pools.ne, pools.bwd_pool != nullptr);
    int &g_attr_bound = g_attr_bound_dev[attr_slot()][ne8];
    const void *fn = ne8 ? reinterpret_cast<const void *>(k_bound<8>) : reinterpret_cast<const void *>(k_bound<4>);
    if ((int)lds > g_attr_bound) {
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        g_attr_bound = (int)lds;
    }
    if (ne8) hipLaunchKernelGGL(k_bound<8>, dim3(n_blocks), dim3(64 * std::min(waves, 8)), lds, static_cast<hipStream_t>(stream), pools);
    else hipLaunchKernelGGL(k_bound<4>, dim3(n_blocks), dim3(64 * waves), lds, static_cast<hipStream_t>(stream), pools);
}

// The launch sequence of one sliced K-bound launch: begin, `iters` x step, the probes, finish.  (Replaying it as a captured hipGraph
// was measured SLOWER than these launches back to back on the stream, tools/bound_rate.py: 39.1 vs 33.3 us per iteration at
// 500 x 5,000; the host's enqueue cost is hidden by enqueueing the K-bound launch behind the next K-search launch, kao_solve.cpp.)
void launch_bound_wide(const BoundPools &pools, const BoundWide &wide, int n_topics, int n_blocks, int waves, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool ne8 = pools.ne == 8;
    const size_t lds = bound_lds_bytes(pools.maxB, 0, pools.maxR, false, pools.ne, pools.bwd_pool != nullptr);
    int &g_attr = g_attr_step_dev[attr_slot()][ne8];
    if ((int)lds > g_attr) {
        (void)hipFuncSetAttribute(ne8 ? reinterpret_cast<const void *>(k_bound_step<8>) : reinterpret_cast<const void *>(k_bound_step<4>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        g_attr = (int)lds;
    }
    hipLaunchKernelGGL(k_bound_begin, dim3((n_topics + 63) / 64), dim3(64), 0, st, pools, wide, n_topics);
    if (ne8) {
        waves = std::min(waves, 8);
        for (int i = 0; i < pools.iters; ++i) hipLaunchKernelGGL(k_bound_step<8>, dim3(n_blocks), dim3(64 * waves), lds, st, pools, wide, 0);
        for (int m = 1; m <= kDualProbes; ++m) hipLaunchKernelGGL(k_bound_step<8>, dim3(n_blocks), dim3(64 * waves), lds, st, pools, wide, m);
    } else {
        for (int i = 0; i < pools.iters; ++i) hipLaunchKernelGGL(k_bound_step<4>, dim3(n_blocks), dim3(64 * waves), lds, st, pools, wide, 0);
        for (int m = 1; m <= kDualProbes; ++m) hipLaunchKernelGGL(k_bound_step<4>, dim3(n_blocks), dim3(64 * waves), lds, st, pools, wide, m);
    }
    hipLaunchKernelGGL(k_bound_finish, dim3(n_topics), dim3(256), 0, st, pools);
}

// One launch of the persistent multi-workgroup driver.  `chunk` partitions per workgroup (BoundWide::chunk); false = the launch
// does not fit this driver (LDS), the caller falls back to launch_bound_wide.
bool launch_bound_multi(const BoundPools &pools, const BoundWide &wide, int n_topics, int n_blocks, int waves, void *stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool ne8 = pools.ne == 8;
    const size_t lds = bound_lds_bytes(pools.maxB, wide.chunk, pools.maxR, true, pools.ne, pools.bwd_pool != nullptr, true);
    if (lds > 160 * 1024) return false;
    static int g_attr_multi_dev[kAttrDevices][2] = {{0}};
    int &g_attr = g_attr_multi_dev[attr_slot()][ne8];
    if ((int)lds > g_attr) {
        (void)hipFuncSetAttribute(ne8 ? reinterpret_cast<const void *>(k_bound_multi<8>) : reinterpret_cast<const void *>(k_bound_multi<4>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        g_attr = (int)lds;
    }
    hipLaunchKernelGGL(k_bound_multi_begin, dim3(n_topics), dim3(256), 0, st, pools, wide);
    if (ne8) hipLaunchKernelGGL(k_bound_multi<8>, dim3(n_blocks), dim3(64 * std::min(waves, 8)), lds, st, pools, wide);
    else hipLaunchKernelGGL(k_bound_multi<4>, dim3(n_blocks), dim3(64 * waves), lds, st, pools, wide);
    hipLaunchKernelGGL(k_bound_finish, dim3(n_topics), dim3(256), 0, st, pools);
    return true;
}

}  // namespace kao
