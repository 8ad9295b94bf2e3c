// kao_search_dev.h -- device-only helpers shared by the K-search family (kao_search.hip: k_search, k_search_curg, k_team, k_init),
// K-canon (kao_canon.hip) and, for band(), K-eval (kao_eval.hip): the words a partition is held in, the per-lane generators, the
// move keys, prices and bands, the topic's register copy, the per-wavefront LDS tables and the passes over them.
// Integer-only, wave64.  The scalar CPU restatement used by the tests is oracle/kao_port.c.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kao_device.h"
#include "kao_internal.h"

namespace kao {

// ------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t xs32(uint32_t &s) {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return s;
}
__device__ __forceinline__ uint32_t mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
__device__ __forceinline__ int band(int c, int lo, int hi) { return max(c - hi, 0) + max(lo - c, 0); }
// band(c+1)-band(c) and band(c-1)-band(c)
__device__ __forceinline__ int dinc(int c, int lo, int hi) { return (int)(c >= hi) - (int)(c < lo); }
__device__ __forceinline__ int ddec(int c, int lo, int hi) { return (int)(c <= lo) - (int)(c > hi); }

// A partition's replica slots as the kernels hold them: NW = 4 words (RF <= 4, one ds_read_b128) or 8 words (RF 5..8, two).
template <int NW> struct alignas(16) Part { uint32_t w[NW]; };
// slot k of a partition, as independent selects (keeps the compiler from building a switch)
__device__ __forceinline__ uint32_t sel4(const Part<4> &a, int k) {
    const uint32_t lo = (k & 2) ? a.w[2] : a.w[0];
    const uint32_t hi = (k & 2) ? a.w[3] : a.w[1];
    return (k & 1) ? hi : lo;
}
__device__ __forceinline__ uint32_t sel4(const Part<8> &a, int k) {
    const uint32_t q0 = (k & 4) ? a.w[4] : a.w[0], q1 = (k & 4) ? a.w[5] : a.w[1], q2 = (k & 4) ? a.w[6] : a.w[2], q3 = (k & 4) ? a.w[7] : a.w[3];
    const uint32_t lo = (k & 2) ? q2 : q0, hi = (k & 2) ? q3 : q1;
    return (k & 1) ? hi : lo;
}
template <int NW> __device__ __forceinline__ void set_slot(Part<NW> &a, int k, uint32_t v) {
#pragma unroll
    for (int i = 0; i < NW; ++i) a.w[i] = (i == k) ? v : a.w[i];
}
// per-lane LCG modulo 2^24: one v_mad_u32_u24 (only the low 24 bits of the state are ever read)
__device__ __forceinline__ uint32_t lcg24(uint32_t &s) {
    // s = (s & 0xFFFFFF) * 0x6D2B79 + 0x3C6EF3; forced to the full-rate 24-bit multiply-add (hipcc otherwise
    // picks the quarter-rate v_mul_lo_u32 for some call sites)
    asm("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(s) : "s"(0x6D2B79u), "v"(0x3C6EF3u));
    return s;
}
// uniform-ish draw on [0, n) from the high bits of a 24x24-bit product: one v_mul_hi_u32_u24.  n8 = n << 8.
__device__ __forceinline__ uint32_t rnd24(uint32_t &s, uint32_t n8) {
    const uint32_t v = lcg24(s);
    return (uint32_t)(((unsigned long long)(v & 0xFFFFFFu) * (unsigned long long)(n8 & 0xFFFFFFu)) >> 32);
}
// same draw for ranges that may exceed 65535 (partition indices): floor(v24 * n / 2^24) = mulhi(v24 << 8, n)
__device__ __forceinline__ uint32_t rnd24_wide(uint32_t &s, uint32_t n) {
    const uint32_t v = lcg24(s);
    return __umulhi((v & 0xFFFFFFu) << 8, n);
}
// A move key: the clamped, biased cost delta above a low byte that breaks ties -- the proposing lane (as it is: < 64) or eight hash bits.
// dP: Lagrangian prices of the broker rows (already in key units) added to the cost by the priced instantiations.
__device__ __forceinline__ uint32_t key_of(int delta, uint32_t low) {
    delta = min(max(delta, -kDBias), kDBias - 2);
    return ((uint32_t)(delta + kDBias) << 8) | low;
}
__device__ __forceinline__ uint32_t make_key_p(int lam, int S, int dV, int dObj, int dP, int lane) { return key_of(__mul24(lam, dV) - __mul24(S, dObj) + dP, (uint32_t)lane); }
__device__ __forceinline__ uint32_t make_key(int lam, int S, int dV, int dObj, int lane) { return key_of(__mul24(lam, dV) - __mul24(S, dObj), (uint32_t)lane); }
__device__ __forceinline__ uint32_t make_key_tie_p(int lam, int S, int dV, int dObj, int dP, uint32_t tie) { return key_of(__mul24(lam, dV) - __mul24(S, dObj) + dP, tie & 0xFFu); }
__device__ __forceinline__ uint32_t make_key_tie(int lam, int S, int dV, int dObj, uint32_t tie) { return key_of(__mul24(lam, dV) - __mul24(S, dObj), tie & 0xFFu); }
// Small-cost launches (search_small_cost, kao_search.hip: the host has shown that no cost of the launch leaves int16): the clamp of
// key_of changes nothing, so a key is the biased cost as it comes out of a chain of 24-bit multiply-adds -- the caller writes the
// cost as lam * dV + S * gain, with whatever part of it is the same for several candidates formed once.
// (as instructions: written with __mul24 and `+` the sums are re-associated and end in v_mul_lo_u32 / v_mad_u64_u32.  mad24s takes a
// wave-uniform factor first; the bias is the addend of the first multiply-add of a chain, so a key is two multiply-adds and a shift-or.)
__device__ __forceinline__ int mad24(int a, int b, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ int mad24s(int s, int b, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "s"(s), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t key_small(int biased_cost, uint32_t low) { return ((uint32_t)biased_cost << 8) | low; }
// Two int16 lanes in one register (the fused scan keeps its two slots' costs in them).  pk_mad_lo: (a.lo * b.lo + c.lo, a.lo * b.hi + c.lo)
// -- a and c broadcast from their low halves, b a wave-uniform pair; pk_mad_s: (a.lo * s.lo + c.lo, a.hi * s.lo + c.hi) -- the
// wave-uniform factor s broadcast from its low half.  16-bit wrap-around, no clamp.
__device__ __forceinline__ uint32_t pk_mad_lo(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_pk_mad_i16 %0, %1, %2, %3 op_sel_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pk_mad_s(uint32_t a, uint32_t s, uint32_t c) {
    uint32_t r;
    asm("v_pk_mad_i16 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(s), "v"(c));
    return r;
}
// pk_mad_s with the factor in a scalar register (the penalty: search_body forms it on the scalar unit); the addend is then a vector
// operand -- a VALU instruction of this ISA reads one scalar register
__device__ __forceinline__ uint32_t pk_mad_ss(uint32_t a, uint32_t s, uint32_t c) {
    uint32_t r;
    asm("v_pk_mad_i16 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(s), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_pk_add_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_pk_sub_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// packed search prices of one broker: low half = replica price a[b], high half = leader price l[b], key units
__device__ __forceinline__ int price_rep(uint32_t pr) { return (int)(short)(pr & 0xFFFFu); }
__device__ __forceinline__ int price_lead(uint32_t pr) { return (int)pr >> 16; }
// Price of one more (p_in) / one fewer (p_out) unit on a priced row whose count is c: the multiplier applies only where the
// count leaves or re-enters its band [lo, hi], i.e. exactly where the violation changes; inside a slack band a unit costs
// nothing (a plain linear term would push the counts of rows with a positive multiplier down to the lower band end).
__device__ __forceinline__ int p_in(int c, int lo, int hi, int price) { return ((c >= hi) | (c < lo)) ? price : 0; }
__device__ __forceinline__ int p_out(int c, int lo, int hi, int price) { return ((c > hi) | (c <= lo)) ? -price : 0; }
// packed broker weights (objective terms per replica / per leader on a broker, kao_topic.broker_w / broker_wl): low | high half
__device__ __forceinline__ int bw_of(uint32_t bw, bool lead) { return (int)(bw & 0xFFFFu) + (lead ? (int)(bw >> 16) : 0); }
// fixed point (kDualScale) -> key units (obj_scale per objective unit), rounded half up, clamped to 16 bits
__device__ __forceinline__ int price_units(int v, int S) { return min(max((S * v + kDualScale / 2) >> kDualLog2, -32767), 32767); }

// NS > 0 (the RF-3 instantiation of k_search): only words 0..NS-1 are compared.  The words beyond hold kNoneW, which equals no
// broker word and whose rack field 0xFFFF equals no rack, so leaving them out changes no result.
template <int NS = 0, int NW> __device__ __forceinline__ bool in4(const Part<NW> &a, uint32_t w) {
    bool r = false;
#pragma unroll
    for (int i = 0; i < (NS ? NS : NW); ++i) r |= a.w[i] == w;
    return r;
}
// replicas of the partition that sit in rack r (empty slots carry rack 0xFFFF and never match)
template <int NS = 0, int NW> __device__ __forceinline__ int cnt4(const Part<NW> &a, uint32_t r) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < (NS ? NS : NW); ++i) n += (int)((a.w[i] >> 16) == r);
    return n;
}
// twice that count: the bit offset of the count's field in a c7_tab (one shift behind the count: summed as selects of 0 / 2 every
// compare's mask is a live scalar pair, and they spill)
template <int NS = 0, int NW> __device__ __forceinline__ int cnt4x2(const Part<NW> &a, uint32_t r) { return cnt4<NS>(a, r) << 1; }
// slot k < NS of a partition: three slots take two selects (the first select passes through an empty asm: selects between words of
// the struct were turned into a dynamically indexed copy of it in scratch; through the asm goes a fresh value, not the three words
// themselves, which stay live and were copied, three v_mov per call)
template <int NS, int NW> __device__ __forceinline__ uint32_t sel_slot(const Part<NW> &a, int k) {
    if constexpr (NS == 3 && NW == 4) {
        int k1 = k & 1, k2 = k & 2;
        asm("" : "+v"(k1), "+v"(k2));
        const uint32_t w0 = a.w[0], w1 = a.w[1], w2 = a.w[2];
        return k2 ? w2 : (k1 ? w1 : w0);
    } else return sel4(a, k);
}

// Row C7 (a partition's replicas per rack, band [prack_lo, prack_hi]) as two bit tables: a count is at most the partition's words, 8,
// so the nine values of dinc and of ddec, signed 2-bit fields, fill 18 bits of a register each and a delta is one v_bfe_i32 of the
// wave-uniform table at twice the count (cnt4x2 counts in twos) -- against two compares, a select and a subtract.
constexpr uint32_t c7_tab(bool dec, int lo, int hi) {
    uint32_t t = 0;
    for (int c = 0; c <= 8; ++c) {
        const int d = dec ? (c <= lo ? 1 : 0) - (c > hi ? 1 : 0) : (c >= hi ? 1 : 0) - (c < lo ? 1 : 0);   // ddec / dinc
        t |= ((uint32_t)d & 3u) << (2 * c);
    }
    return t;
}
__device__ __forceinline__ int c7_delta(uint32_t tab, int cnt2) { return __builtin_amdgcn_sbfe((int)tab, (unsigned)cnt2, 2u); }

struct TopicRegs {  // wave-uniform copy of the fields the inner loop needs
    int P, RF, R, m, Bx;
    uint32_t magic;
    int rep_lo, rep_hi, lead_lo, lead_hi, rack_lo, rack_hi, prack_lo, prack_hi;
    int w00, w01, w10, w11;
    uint32_t c7_inc, c7_dec;   // c7_tab of [prack_lo, prack_hi]
};

template <int RFT = 0> __device__ __forceinline__ TopicRegs topic_regs(const TopicDev *TD) {   // RFT > 0: the replication factor of every topic of the launch
    TopicRegs T;
    T.P = TD->P; T.RF = RFT ? RFT : TD->RF; T.R = TD->R; T.m = TD->m; T.Bx = TD->Bx; T.magic = TD->magic;
    T.rep_lo = TD->rep_lo; T.rep_hi = TD->rep_hi; T.lead_lo = TD->lead_lo; T.lead_hi = TD->lead_hi;
    T.rack_lo = TD->rack_lo; T.rack_hi = TD->rack_hi; T.prack_lo = TD->prack_lo; T.prack_hi = TD->prack_hi;
    T.w00 = TD->w00; T.w01 = TD->w01; T.w10 = TD->w10; T.w11 = TD->w11;
    T.c7_inc = c7_tab(false, T.prack_lo, T.prack_hi); T.c7_dec = c7_tab(true, T.prack_lo, T.prack_hi);
    return T;
}

// objective weight of broker word w on a partition whose current replicas are c, in new role nr
// (NS as in in4: words 0..NS-1 only)
template <int NS = 0, int NW> __device__ __forceinline__ int role_w2(const Part<NW> &c, uint32_t w, int wl, int wf) {
    bool fol = false;
#pragma unroll
    for (int i = 1; i < (NS ? NS : NW); ++i) fol |= c.w[i] == w;
    return (c.w[0] == w) ? wl : (fol ? wf : 0);
}
template <int NS = 0, int NW> __device__ __forceinline__ int role_w(const TopicRegs &T, const Part<NW> &c, uint32_t w, int nr) {
    return role_w2<NS>(c, w, nr ? T.w01 : T.w00, nr ? T.w11 : T.w10);
}
// internal index -> LDS word (x | rack << 16); 0xFFFF -> empty
__device__ __forceinline__ uint32_t to_word(const TopicRegs &T, uint32_t x) {
    return x == 0xFFFFu ? kNoneW : (x | (mulhi(x, T.magic) << 16));
}
// a restart's state in HBM between launches (LDS path): NW x u16 internal indices per partition
template <int NW> __device__ __forceinline__ Part<NW> load_packed(const TopicRegs &T, const unsigned char *base, int p) {
    Part<NW> a;
    if (NW == 4) {
        const uint2 s = reinterpret_cast<const uint2 *>(base)[p];
        a.w[0] = to_word(T, s.x & 0xFFFFu); a.w[1] = to_word(T, s.x >> 16); a.w[2] = to_word(T, s.y & 0xFFFFu); a.w[3] = to_word(T, s.y >> 16);
    } else {
        const uint4 s = reinterpret_cast<const uint4 *>(base)[p];
        const uint32_t v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int i = 0; i < NW / 2; ++i) { a.w[2 * i] = to_word(T, v[i & 3] & 0xFFFFu); a.w[2 * i + 1] = to_word(T, v[i & 3] >> 16); }
    }
    return a;
}
template <int NW> __device__ __forceinline__ void store_packed(unsigned char *base, int p, const Part<NW> &a) {
    if (NW == 4) reinterpret_cast<uint2 *>(base)[p] = make_uint2((a.w[0] & 0xFFFFu) | (a.w[1] << 16), (a.w[2] & 0xFFFFu) | (a.w[3] << 16));
    else reinterpret_cast<uint4 *>(base)[p] = make_uint4((a.w[0] & 0xFFFFu) | (a.w[1] << 16), (a.w[2] & 0xFFFFu) | (a.w[3] << 16),
                                                         (a.w[4 % NW] & 0xFFFFu) | (a.w[5 % NW] << 16), (a.w[6 % NW] & 0xFFFFu) | (a.w[7 % NW] << 16));
}
// sum over all R racks of band(#replicas of the partition in the rack)
template <int NW> __device__ __forceinline__ int part_rack_viol(const TopicRegs &T, const Part<NW> &a) {
    int s = 0, touched = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const uint32_t rk = a.w[k] >> 16;
        bool first = a.w[k] != kNoneW;
#pragma unroll
        for (int j = 0; j < k; ++j) first &= (a.w[j] >> 16) != rk;   // this rack has not been counted yet
        if (first) { s += band(cnt4(a, rk), T.prack_lo, T.prack_hi); touched++; }
    }
    return s + (T.R - touched) * T.prack_lo;  // band(0, lo, hi) == lo
}

// ------------------------------------------------------------------------------------------------
// K-search
// ------------------------------------------------------------------------------------------------
constexpr int kTeamRec = 12;   // ints per proposal record of a team (search_body, kTeam)
template <int NW> struct WaveLds {
    Part<NW> *A;  // [P] this restart's assignment, NW words per partition
    uint32_t *C;  // [Bx] replicas | leaders << 16 per broker
    uint16_t *W;  // [Bx] band state of every broker, derived from C and kept current with it (see band_fields); bit 15 = no candidate
    int *K;       // [krt] replicas per rack (krt = search_rack_tab(largest rack count of the launch group))
    int *RT;      // [krt] scratch: rack-dependent part of a REPLACE delta for the slot being scanned
};

// Band state of one broker, precomputed from its counter word c = replicas | leaders << 16 so that delta evaluation costs
// one v_bfe_i32 per row instead of two compares, a select and a subtract.  Replica row (C3) in bits 5:0, leader row (C4) in
// bits 11:6, each: signed 2-bit dinc = band(c + 1) - band(c), signed 2-bit ddec = band(c - 1) - band(c) (README.md:158-166),
// and the two flags that say where a search price applies (p_in / p_out).  Bit 15 marks an index that is no candidate: padding
// slots of the rack-major index space always, and during a REPLACE scan the brokers already in the partition (row C5,
// README.md:168-171).
constexpr int kWIncR = 0, kWDecR = 2, kWPinR = 4, kWPoutR = 5, kWIncL = 6, kWDecL = 8, kWPinL = 10, kWPoutL = 11;
__device__ __forceinline__ int wfld(uint32_t w, int off) { return __builtin_amdgcn_sbfe((int)w, (unsigned)off, 2u); }
__device__ __forceinline__ int wfldw(uint32_t w, int off, uint32_t width) { return __builtin_amdgcn_sbfe((int)w, (unsigned)off, width); }   // width 0 -> 0
__device__ __forceinline__ int wflag(uint32_t w, int off) { return __builtin_amdgcn_sbfe((int)w, (unsigned)off, 1u); }                      // all ones / 0
__device__ __forceinline__ int wflagw(uint32_t w, int off, uint32_t width) { return __builtin_amdgcn_sbfe((int)w, (unsigned)off, width); }
// The six state bits of one band row as a function of where the count c stands: a = clamp(c - lo, -1, 1), b = clamp(c - hi, -1, 1)
//   dinc = (c >= hi) - (c < lo) = (b >= 0) - (a < 0)        ddec = (c <= lo) - (c > hi) = (a <= 0) - (b > 0)
//   pin  = (c >= hi) | (c < lo)   (one more unit leaves / re-enters the band: where a price applies, p_in)
//   pout = (c > hi) | (c <= lo)   (one fewer unit, p_out)
// entry = dinc & 3 | (ddec & 3) << 2 | pin << 4 | pout << 5, nine entries of 6 bits indexed by 3 * (a + 1) + (b + 1) in one 64-bit constant.
constexpr unsigned long long band_entry_of(int a, int b) {
    const int di = (b >= 0 ? 1 : 0) - (a < 0 ? 1 : 0), dd = (a <= 0 ? 1 : 0) - (b > 0 ? 1 : 0);
    const int pin = (b >= 0 || a < 0) ? 1 : 0, pout = (b > 0 || a <= 0) ? 1 : 0;
    return (unsigned long long)((di & 3) | ((dd & 3) << 2) | (pin << 4) | (pout << 5));
}
constexpr unsigned long long band_table() {
    unsigned long long t = 0;
    for (int a = -1; a <= 1; ++a) for (int b = -1; b <= 1; ++b) t |= band_entry_of(a, b) << (6 * (3 * (a + 1) + (b + 1)));
    return t;
}
constexpr unsigned long long kBandTab = band_table();
// clamp(x, -1, 1) as one v_med3_i32 (written as min / max it is recognised as a three-way compare and becomes two compares
// and two selects, eight of the twelve instructions of a band_entry)
__device__ __forceinline__ int clamp_pm1(int x) {
    int r;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ uint32_t band_entry(int c, int lo, int hi) {
    const int a = clamp_pm1(c - lo), b = clamp_pm1(c - hi);
    int t;   // 3 a + b, then the shift 6 t + 24, as 24-bit multiply-adds (on a value out of an asm a plain `*` and `+` become a v_mad_u64_u32)
    asm("v_mad_i32_i24 %0, %1, 3, %2" : "=v"(t) : "v"(a), "v"(b));
    return (uint32_t)(kBandTab >> (uint32_t)(__mul24(t, 6) + 24)) & 63u;
}
// The same entry as a lookup.  Which of the nine combinations (a, b) a count stands for depends only on where it stands against
// [lo, hi], so a row with a narrow band gets a table of its own, built once per launch: entry i = band_entry of the count lo - 1 + i
// (i = 0: below the band, i = 1: at lo, ..., i = hi - lo + 2: above it), six bits each, and every entry behind the last one repeats
// it -- the index is then clamped to the same [0, kBandTabLast] for every band and a row costs three instructions, the multiply-add
// 6 c + (6 - 6 lo), a v_med3_i32 with two inline constants and a v_bfe_u32, against band_entry's eight.  kBandTabLast + 1 = 5 entries
// fill one 32-bit register: bands with hi - lo <= 2 (a balanced topic has hi - lo <= 1; wider ones come from bounds_override).  Wider
// bands keep band_entry, the same function (the host picks per launch group, search_band_tabs; tests/test_gpu_search_tables.py walks
// both over every band).
constexpr int kBandTabLast = 4;
constexpr bool band_tab_fits(int lo, int hi) { return lo >= 0 && lo <= hi && hi <= 0xFFFF && hi - lo + 2 <= kBandTabLast; }
constexpr uint32_t band_tab(int lo, int hi) {
    uint32_t t = 0;
    for (int i = 0; i <= kBandTabLast; ++i) {
        const int c = lo - 1 + (i < hi - lo + 2 ? i : hi - lo + 2);
        const int a = c < lo ? -1 : (c > lo ? 1 : 0), b = c < hi ? -1 : (c > hi ? 1 : 0);
        t |= (uint32_t)band_entry_of(a, b) << (6 * i);
    }
    return t;
}
constexpr int band_tab_bias(int lo) { return 6 - 6 * lo; }
// the lookup as plain arithmetic (the host's restatement of band_lookup, for the tests: kao_search_band_row)
constexpr uint32_t band_lookup_plain(int c, int bias, uint32_t tab) {
    const int x = 6 * c + bias;
    return (tab >> (x < 0 ? 0 : (x > 6 * kBandTabLast ? 6 * kBandTabLast : x))) & 63u;
}
__device__ __forceinline__ uint32_t band_lookup(int c, int bias, uint32_t tab) {
    int x;
    asm("v_mad_i32_i24 %0, %1, 6, %2\n\tv_med3_i32 %0, %0, 0, 24" : "=&v"(x) : "v"(c), "v"(bias));
    static_assert(6 * kBandTabLast == 24, "the clamp's inline constant");
    return __builtin_amdgcn_ubfe(tab, (uint32_t)x, 6u);
}
// a row by the form the instantiation holds (search_body): r0, r1 = bias, table (kTab) or lo, hi
template <bool kTab> __device__ __forceinline__ uint32_t band_row(int c, int r0, int r1) {
    if constexpr (kTab) return band_lookup(c, r0, (uint32_t)r1);
    else return band_entry(c, r0, r1);
}
__device__ __forceinline__ uint32_t band_fields(const TopicRegs &T, uint32_t c) {
    return band_entry((int)(c & 0xFFFFu), T.rep_lo, T.rep_hi) | (band_entry((int)(c >> 16), T.lead_lo, T.lead_hi) << 6);
}
constexpr uint32_t kWRowR = 0x003Fu, kWRowL = 0x0FC0u;   // the replica row (C3) and the leader row (C4) of a band-state word
constexpr uint32_t kWNoCand = 0x8000u;
// Bit 14: no candidate for the SECOND slot of a fused two-slot REPLACE scan (search_body), which marks the brokers of its two partitions
// at once, each slot with its own bit.  Padding indices carry both bits.
constexpr uint32_t kWNoCand2 = 0x4000u;
// W[x] for every index of the topic (XR: rack of x, `inv` = padding)
// (`lane`, `stride`: a wavefront strides by 64; the wavefronts of a team stride together by the workgroup size)
template <int NW> __device__ __forceinline__ void rebuild_band_state(const TopicRegs &T, const WaveLds<NW> &L, const uint8_t *XR, uint32_t inv, int lane, int stride = 64) {
    for (int x = lane; x < ((T.Bx + 63) & ~63); x += stride) L.W[x] = (uint16_t)(XR[x] == inv ? (kWNoCand | kWNoCand2) : band_fields(T, L.C[x]));
}

// ------------------------------------------------------------------------------------------------
// Hole filling of an initialising launch in band-state form (search_body's `init == 1` block; specification: oracle/kao_port.c::ls_init).
// A hole (p,k) takes the valid broker outside the partition with the lowest lam_max * dV - S * dObj of its insertion, ties by eight
// hashed bits, then the lowest lane, then the earliest round.  The scan has the form of the iteration loop's one-slot REPLACE scan:
// the brokers of the partition carry kWNoCand in W (the caller marks them, fill_mark / fill_unmark), the rack-dependent part of the
// delta comes out of a table built once per hole, and a candidate costs one W read, one RT read, two bit-field extracts, a
// multiply-add, the hash and the key; the running minimum is one v_min_u32.  The tables come by pointer, so that k_init can take the
// helper over once its LDS carve holds a W.
// ------------------------------------------------------------------------------------------------
struct FillTabs {
    uint16_t *W;          // [Bx to 64] band state, current with C; the partition's brokers marked kWNoCand
    const uint8_t *XR;    // [Bx to 64] rack of index x, padding: the spare entry krt - 1
    const int *K;         // [krt] replicas per rack
    int *RT;              // [krt] the hole's rack table; RT[krt - 1] == 0 (the caller's)
    const uint32_t *PR;   // priced: packed broker prices
    const int *PG;        //         rack prices
    const uint32_t *BW;   //         broker weights (nullptr: none)
};
constexpr uint32_t kFillTieStep = 0x165667B1u;   // the tie hash of index x is fmix32(hmix + x * kFillTieStep) >> 24
// lane i < NS looks after word i of the partition: its broker is no candidate (row C5) while the partition's holes are filled.  The
// marks come off by clearing the bit -- a valid index carries it for no other reason -- on the words as they are AFTER the fill, so
// the winners, whose rows fill_insert has written with the mark, lose it too and keep their updated rows.
template <int NS, int NW> __device__ __forceinline__ void fill_mark(uint16_t *W, const Part<NW> &a, int lane) {
    const uint32_t ai = sel_slot<NS>(a, lane & (NW - 1));
    if ((lane < NS) & (ai != kNoneW)) W[ai & 0xFFFFu] |= (uint16_t)kWNoCand;
}
template <int NS, int NW> __device__ __forceinline__ void fill_unmark(uint16_t *W, const Part<NW> &a, int lane) {
    const uint32_t ai = sel_slot<NS>(a, lane & (NW - 1));
    if ((lane < NS) & (ai != kNoneW)) W[ai & 0xFFFFu] &= (uint16_t)~kWNoCand;
}
// RT[r] = what one more replica in rack r does to the rack's total (C6) and to the partition's count in it (C7); priced: that
// violation delta in the low byte, the rack's price -- where its total leaves or re-enters the band -- above it, as in the REPLACE scan
template <int NS, bool kPriced, int NW> __device__ __forceinline__ void fill_rack_table(const TopicRegs &T, const FillTabs &F, const Part<NW> &a, int lane) {
    for (int r = lane; r < T.R; r += 64) {
        const int kr = F.K[r];
        int v = dinc(kr, T.rack_lo, T.rack_hi) + c7_delta(T.c7_inc, cnt4x2<NS>(a, (uint32_t)r));
        if (kPriced) v = (v & 0xFF) | (p_in(kr, T.rack_lo, T.rack_hi, F.PG[r]) * 256);
        F.RT[r] = v;
    }
}
// One round: the key of candidate x, (cost + bias) << 16 | tie << 8 | rd, cost field 0xFFFF where x is no candidate (W's bit 15,
// sign-extended).  `h` = hmix + x * kFillTieStep.  fmix32's last xor-shift does not reach bits 31:24 and is left out.
// kClamp = false: small-cost launches.  A hole's cost is lam_max * dV with 0 <= |dV| <= 4 (replica row, leader row, rack total, the
// partition's count in the rack) and no objective term (kWithW is false there), inside search_small_cost's 8 lam_max + 4 S w_max.
// The round's loads come in: `w` = W[x] sign-extended, `r` = XR[x], `rt` = RT[r].  A trip of two rounds issues its W / XR reads together
// and its RT reads together (fill_hole): the wavefront waits for two dependent LDS round trips per pair, not four.
template <int NS, bool kPriced, bool kClamp, bool kWithW, int NW>
__device__ __forceinline__ uint32_t fill_round_on(const TopicRegs &T, const FillTabs &F, const Part<NW> &c, int x, int rd, uint32_t h, int lam, int S, bool lead, int w, uint32_t r, int rt) {
    const uint32_t lw = lead ? 2u : 0u, lf = lead ? 1u : 0u;   // widths of the leader field / flag: zero for follower holes
    int cost;
    if (kPriced) {
        const uint32_t prx = F.PR[x];
        const int dVx = wfld(w, kWIncR) + wfldw(w, kWIncL, lw) + (int)(signed char)(rt & 0xFF);
        cost = __mul24(lam, dVx) + kDBias + (rt >> 8) + (wflag(w, kWPinR) & price_rep(prx)) + (wflagw(w, kWPinL, lf) & price_lead(prx));
        if (F.BW) cost -= __mul24(S, bw_of(F.BW[x], lead));
    } else {
        cost = mad24s(lam, wfld(w, kWIncR) + wfldw(w, kWIncL, lw) + rt, kDBias);
    }
    if (kWithW) cost -= __mul24(S, role_w2<NS>(c, (uint32_t)x | (r << 16), lead ? T.w00 : T.w01, lead ? T.w10 : T.w11));
    if (kClamp) cost = min(max(cost, 0), 2 * kDBias - 2);
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u;
    return ((uint32_t)cost << 16) | ((h >> 16) & 0xFF00u) | (uint32_t)rd | ((uint32_t)w & 0xFFFF0000u);
}
template <int NS, bool kPriced, bool kClamp, bool kWithW, int NW>
__device__ __forceinline__ uint32_t fill_round(const TopicRegs &T, const FillTabs &F, const Part<NW> &c, int x, int rd, uint32_t h, int lam, int S, bool lead) {
    const int w = (int)reinterpret_cast<const short *>(F.W)[x];
    const uint32_t r = F.XR[x];
    return fill_round_on<NS, kPriced, kClamp, kWithW>(T, F, c, x, rd, h, lam, S, lead, w, r, F.RT[r]);
}
// One hole of partition words `a` (current words `c`): the winner's word x | rack << 16, wave-uniform; kNoneW when no index is a
// candidate (fewer valid brokers than replicas: the model refuses such a topic).
// kWeights: a candidate has an objective weight only as a current replica of the partition that is not in `a`; the rounds that hold
// one (at most NS) are scored through the kWithW body.  False for the RF-3 instantiation: `a` starts as the current words and the
// fill only adds, so every current replica is in `a` and marked.
template <int NS, bool kPriced, bool kClamp, bool kWeights, int NW>
__device__ __forceinline__ uint32_t fill_hole(const TopicRegs &T, const FillTabs &F, const Part<NW> &a, const Part<NW> &c, bool lead, uint32_t hmix, int lam, int S, int lane) {
    fill_rack_table<NS, kPriced>(T, F, a, lane);
    int mr[NS] = {};
    if constexpr (kWeights) {
        const uint32_t ci = sel_slot<NS>(c, lane & (NW - 1));
        const int mr_l = ((lane < NS) & (ci != kNoneW) & !in4<NS>(a, ci)) ? (int)((ci & 0xFFFFu) >> 6) : -1;
#pragma unroll
        for (int i = 0; i < NS; ++i) mr[i] = __builtin_amdgcn_readlane(mr_l, i);
    }
    uint32_t h = hmix + (uint32_t)lane * kFillTieStep;
    uint32_t best = kKeyNull;
    int chunk = 0;
    for (int cb = 0; cb < T.Bx; cb += 16384) {   // the key holds the round in eight bits: chunks of 256 rounds
        uint32_t bestc = kKeyNull;
        const int n_rd = (min(T.Bx, cb + 16384) - cb + 63) >> 6;
        int rd = 0, x = cb + lane;
        if constexpr (!kWeights) {
            for (; rd + 1 < n_rd; rd += 2, x += 128, h += 128u * kFillTieStep) {   // two rounds share the address arithmetic and one v_min3_u32
                const int wa = (int)reinterpret_cast<const short *>(F.W)[x], wb = (int)reinterpret_cast<const short *>(F.W)[x + 64];
                const uint32_t ra = F.XR[x], rb = F.XR[x + 64];
                const int rta = F.RT[ra], rtb = F.RT[rb];
                const uint32_t k0 = fill_round_on<NS, kPriced, kClamp, false>(T, F, c, x, rd, h, lam, S, lead, wa, ra, rta);
                const uint32_t k1 = fill_round_on<NS, kPriced, kClamp, false>(T, F, c, x + 64, rd + 1, h + 64u * kFillTieStep, lam, S, lead, wb, rb, rtb);
                bestc = min(bestc, min(k0, k1));
            }
            if (rd < n_rd) { bestc = min(bestc, fill_round<NS, kPriced, kClamp, false>(T, F, c, x, rd, h, lam, S, lead)); h += 64u * kFillTieStep; }
        } else {
            for (; rd < n_rd; ++rd, x += 64, h += 64u * kFillTieStep) {
                bool wgt = false;   // wave-uniform
#pragma unroll
                for (int i = 0; i < NS; ++i) wgt |= mr[i] == (cb >> 6) + rd;
                bestc = min(bestc, wgt ? fill_round<NS, kPriced, kClamp, true>(T, F, c, x, rd, h, lam, S, lead) : fill_round<NS, kPriced, kClamp, false>(T, F, c, x, rd, h, lam, S, lead));
            }
        }
        if ((bestc >> 8) < (best >> 8)) { best = bestc; chunk = cb; }   // strict: ties stay with the earlier round
    }
    // one reduction: (cost, tie) << 7 | lane -- lowest key, then lowest lane; the round is read from the winner's lane
    const uint32_t m = wave_umin(((best >> 1) & ~127u) | (uint32_t)lane);
    if ((m >> 15) == 0xFFFFu) return kNoneW;
    const int win = (int)(m & 63u);
    const uint32_t bw = (uint32_t)__builtin_amdgcn_readlane((int)best, win);
    const uint32_t xs = (uint32_t)__builtin_amdgcn_readlane(chunk, win) + ((bw & 255u) << 6) + (uint32_t)win;
    return xs | ((uint32_t)F.XR[xs] << 16);
}

// rebuild C and K from A (lanes stride partitions; LDS atomics)
// (a team calls it between two workgroup barriers and zeroes, then counts, with a barrier in between: `stride` > 64)
template <int NW> __device__ __forceinline__ void recount(const TopicRegs &T, const WaveLds<NW> &L, int lane, int stride, int krt) {
    for (int x = lane; x < ((T.Bx + 63) & ~63); x += stride) L.C[x] = 0;
    for (int r = lane; r < krt; r += stride) L.K[r] = 0;
    if (stride > 64) __syncthreads();
    for (int p = lane; p < T.P; p += stride) {
        const Part<NW> a = L.A[p];
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (a.w[k] != kNoneW) { atomicAdd(&L.C[a.w[k] & 0xFFFFu], k == 0 ? 0x10001u : 1u); atomicAdd(&L.K[a.w[k] >> 16], 1); }
    }
}

// total violation magnitude and objective of the state in LDS (C, K must be current)
// kTeam: the wavefronts of the workgroup split the passes and meet through `TS` (two ints per wavefront); every wavefront
// returns the totals.  Integer sums: the split changes no result.
template <int NW, bool kTeam = false> __device__ __forceinline__ void full_cost(const TopicRegs &T, const WaveLds<NW> &L, const Part<NW> *CUR, const int *RSZ,
                                                            int lane, int stride, int &V, int &obj, const uint32_t *BW = nullptr,
                                                            int *TS = nullptr, int wave = 0, int n_waves = 1) {
    int v = 0, o = 0;
    for (int p = lane; p < T.P; p += stride) {
        const Part<NW> a = L.A[p];
        const Part<NW> c = CUR[p];
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (a.w[k] != kNoneW) o += role_w(T, c, a.w[k], k == 0 ? 0 : 1);
        v += part_rack_viol(T, a);
    }
    for (int x = lane; x < T.Bx; x += stride) {
        const int r = (int)mulhi((uint32_t)x, T.magic);
        if (x - r * T.m < RSZ[r]) {
            const uint32_t c = L.C[x];
            v += band((int)(c & 0xFFFFu), T.rep_lo, T.rep_hi) + band((int)(c >> 16), T.lead_lo, T.lead_hi);
            if (BW) { const uint32_t bw = BW[x]; o += (int)(c & 0xFFFFu) * (int)(bw & 0xFFFFu) + (int)(c >> 16) * (int)(bw >> 16); }
        }
    }
    for (int r = lane; r < T.R; r += stride) v += band(L.K[r], T.rack_lo, T.rack_hi);
    V = wave_sum(v);
    obj = wave_sum(o);
    if (kTeam) {
        __syncthreads();   // (TS may still be read from the previous call)
        if ((lane & 63) == 0) { TS[2 * wave] = V; TS[2 * wave + 1] = obj; }
        __syncthreads();
        int tv = 0, to = 0;
        if ((lane & 63) < n_waves) { tv = TS[2 * (lane & 63)]; to = TS[2 * (lane & 63) + 1]; }
        V = wave_sum(tv);
        obj = wave_sum(to);
    }
}

// (the trip count is wave-uniform and the lanes beyond P sit out inside the body: with `p = lane; p < P` as the loop's own bound the
//  caller's "is this a new best" branch was merged with a per-lane one, and what it sets -- best_obj -- stopped being a scalar)
template <int NW> __device__ __forceinline__ void snapshot(const TopicRegs &T, const WaveLds<NW> &L, const uint16_t *ext, uint16_t *best, int lane, int stride = 64) {
    int p0 = 0;
    do {   // (bottom-tested: a topic has a partition, and the lanes beyond P sit out anyway -- a top-tested loop keeps its guard `P < 1` as a
           //  scalar pair across the iteration loop, which has none to spare)
        const int p = p0 + lane;
        if (p < T.P) {
            const Part<NW> a = L.A[p];
            uint16_t *o = best + p * T.RF;
#pragma unroll
            for (int k = 0; k < NW; ++k)
                if (k < T.RF) o[k] = ext[a.w[k] & 0xFFFFu];
        }
        p0 += stride;
    } while (p0 < T.P);
}

}  // namespace kao
