// kao_search.hip -- the K-search family (gfx950): parallel-restart local search "KAO-LS"  and its launchers.
//   k_search      : one wavefront owns one restart.  Per iteration its 64 lanes either score random slots (tournament) and then scan
//                   every target broker / partner slot for the winning slot, or sample their own proposals; every neighbour is
//                   delta-evaluated for feasibility (C3,C4,C6,C7; C1,C2,C5 hold by construction) and move cost against broker / rack
//                   tables staged in LDS; a DPP min-reduce over the wavefront picks the move.  k_search<false> also keeps the
//                   assignment words in LDS; k_search<true> leaves them in HBM/L2 for topics that do not fit.
//                   An initialising launch first fills the holes of the current assignment by best insertion, scored from the same
//                   band state the loop scans with: W is built in front of the fill, the partition's brokers are marked in it, a
//                   rack table is built per hole and the winner's counters and band rows are updated at once (fill_hole,
//                   kao_search_dev.h), so the loop starts from the W the fill leaves.
//   k_search_curg : working assignment in LDS, current assignment from global memory.
//   k_team        : the wavefronts of a workgroup as a team on ONE restart (topics in global memory).
//   k_init        : the hole filling of an initialising launch, one workgroup per restart (topics in global memory).
// All but k_init are instantiations of search_body.  Integer-only, wave64, no MFMA.  The scalar CPU restatement is oracle/kao_port.c.
#include "kao_search_dev.h"

#include <map>
#include <mutex>
#include <tuple>

namespace kao {

// kGlobalA = false: the restart's assignment words and the topic's current-assignment words are staged in LDS
//                   (topics that fit: the fast path).
// kGlobalA = true : they stay in global memory (HBM / L2) -- 16 B per partition per restart, updated in place --
//                   and only the broker / rack tables live in LDS.  Same algorithm, same results; this is what
//                   lets a single 100k-partition topic run.
// kCurG = true  : (kGlobalA = false only; round 5) the restart's WORKING assignment words live in LDS, the topic's CURRENT-assignment
//                   words are read from global memory (one copy per topic, shared by every restart: it sits in L2).  Holding both in LDS
//                   costs 2 x 16 B per partition, so a restart fitted 160 KiB only up to ~4,900 partitions and 500 x 5000 ran the HBM
//                   path at 4.8 ms a launch; with the working words alone the limit is ~9,800.  Same arithmetic: the replay holds.
// kPriced = true : the cost of a move also carries Lagrangian PRICES of the coupling rows (K-bound's multipliers: replicas
//                   per broker / rack, leaders per broker) -- an augmented-Lagrangian search: with near-optimal prices the
//                   chain steps an improvement needs (objective down a little, violation unchanged) become neutral moves.
// NW              : replica words per partition -- 4 (RF and current RF <= 4) or 8 (up to 8 replicas).
// kWide          : the launch group holds topics of 512 replica slots or more: their tournament scores several slots per lane
//                   and is issued two slots per trip, the REPLACE scan two rounds per trip (instruction-level parallelism for
//                   the one-wavefront-per-SIMD regime of large topics; costs registers the small-topic instantiation keeps)
// kTeam = true  : (topics in global memory only; kernel k_team) the wavefronts of the workgroup are a TEAM on ONE restart: they
//                   share one set of counters and band states in LDS, every wavefront proposes its own move per iteration against
//                   the same frozen state, and a proposal is applied iff it is acceptable and shares no partition, broker or
//                   (when it changes rack totals) rack with an acceptable proposal of a lower-numbered wavefront -- disjoint
//                   moves commute, so violation and objective deltas add up.  A 30,000-partition topic gets W moves per
//                   latency-bound iteration instead of one (the depth large topics lack), deterministically (specification:
//                   oracle/kao_port.c::ls_run with team > 1, replayed bit for bit).
// RFT = 3        : (LDS-resident, NW = 4) every topic of the launch has RF 3 and at most 3 current replicas per partition, so word 3 of
//                   both the working and the current words is always kNoneW (no move writes a slot k >= RF).  The move arithmetic
//                   visits words 0..2 only and the slot loops run 2 / 3 times without `k >= RF` guards; memory layout and results
//                   are those of RFT = 0 (RF read per topic).
// kSmall         : (RFT = 3 only) the host has shown that no cost this launch forms leaves int16 (search_small_cost below): the keys
//                   are multiply-adds without the clamp, and the fused scan keeps its two slots' costs in the halves of one register
//                   (v_pk_mad_i16 / v_pk_add_i16), the penalty's parameters come out of one packed scalar and a broker's band rows out
//                   of per-topic tables (the host has also shown that every band fits one: search_band_tabs).  Same draws, keys,
//                   winners, stores and counters as kSmall = false.
// What one workgroup runs of a launch: everything (whole_launch) or one chunk of a chunked launch (chunk_take, below).  A chunk other than
// the first is the launch carried on -- the non-initialising prologue without the elite rule, the generator words of the chunk before
// it, its own range of iterations.
struct SearchPiece {
    uint32_t entry;      // index into the block map (the whole launch: blockIdx.x)
    int32_t init, elite; // SearchParams::init / elite as this piece sees them (a later chunk: 0)
    uint32_t first, n;   // its iterations: first .. first + n - 1 of the launch's
    bool later;          // a chunk behind the first: per-lane generator words from SearchPools::chunk_rng, no re-keying
    uint32_t ticket;     // chunked launches: the workgroup's ticket
};
__device__ __forceinline__ void chunk_pass(uint32_t ticket);
// A kernel argument read where it is used, behind the iteration loop: taken from `pl` / `prm` there it is loaded with the others in
// front of the loop and stays live across it -- in kernels whose scalar file is full and whose vector file has no register to spare
// (the k_search kernels take SearchPools, then SearchParams: the kernel-argument segment holds them in that order).
template <class T> __device__ __forceinline__ T late_kernarg(size_t off) {
    auto p = (const __attribute__((address_space(4))) unsigned char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *reinterpret_cast<const __attribute__((address_space(4))) T *>(p + off);
}
static_assert(sizeof(SearchPools) % alignof(SearchParams) == 0, "late_kernarg: SearchParams follows SearchPools without padding");
constexpr size_t kArgPrm = sizeof(SearchPools);
// a record of the chunk schedule (host-written: through the constant address space, a scalar load)
__device__ __forceinline__ int4 sched_record(const int4 *sched, uint32_t ticket) {
    auto p = (const __attribute__((address_space(4))) int *)sched + 4 * (size_t)ticket;
    return make_int4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ SearchPiece whole_launch(const SearchParams &prm) { return SearchPiece{blockIdx.x, prm.init, prm.elite, 0u, prm.iters, false, 0u}; }

// kChunked        : (LDS-resident, no team, not kCurG) the instantiation a chunked launch runs: the workgroup's piece comes from
//                   chunk_take, not from blockIdx.x and the launch parameters.  Launches in one piece run kChunked = false, whose code
//                   takes nothing from `pc`.
template <bool kGlobalA, bool kPriced, int NW, bool kWide, bool kTeam, bool kCurG = false, int RFT = 0, bool kSmall = false, bool kChunked = false>
__device__ __forceinline__ void search_body(unsigned char *smem, const SearchPools &pl, const SearchParams &prm, const SearchPiece pc) {
    static_assert(!kChunked || (!kGlobalA && !kTeam && !kCurG), "chunked launches: LDS-resident topics, one wavefront per restart");
    static_assert(!kTeam || kGlobalA, "teams run topics that live in global memory");
    constexpr bool kCanChunk = kChunked;
    const uint32_t pc_entry = kChunked ? pc.entry : blockIdx.x;
    const int32_t pc_init = kChunked ? pc.init : prm.init, pc_elite = kChunked ? pc.elite : prm.elite;
    static_assert(!kCurG || !kGlobalA, "kCurG: the working assignment is in LDS");
    static_assert(RFT == 0 || (RFT == 3 && NW == 4 && !kGlobalA && !kTeam), "RFT = 3: LDS-resident topics of four words per partition");
    static_assert(!kSmall || (RFT == 3 && !kPriced && !kCurG), "kSmall: the unpriced RF-3 instantiation");
    constexpr int NS = RFT ? RFT : NW;   // words of a partition the move arithmetic visits
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = kTeam ? __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6)) : 1;   // team size W
    const int tid = kTeam ? (int)threadIdx.x : lane, nthr = kTeam ? (int)blockDim.x : 64;   // who strides the O(P) / O(B) passes
    // The chunk-capable instantiations read the block map through the constant address space: a scalar load whatever stands in front
    // of it.  (Left to itself the compiler issues a scalar load only where it can show that nothing in the kernel wrote the location
    // before; behind the ticket's atomics it cannot.  The map is written by the host alone.  The topic's descriptor is NOT read that
    // way: its loads then count as invariant, are kept across the iteration loop instead of repeated behind it, and the loop paid
    // 4 % in restored scalars -- docs/notes_r16.md.)
    using MapPtr = std::conditional_t<kCanChunk, const __attribute__((address_space(4))) int *, const int *>;
    int2 bm;
    if constexpr (kChunked) bm = make_int2(((MapPtr)pl.block_map)[2 * pc_entry], ((MapPtr)pl.block_map)[2 * pc_entry + 1]);
    else bm = pl.block_map[pc_entry];
    const TopicDev *TD = pl.topics + bm.x;

    TopicRegs T = topic_regs<RFT>(TD);
    // both C7 tables are formed here, once: the hole filling reads c7_inc, the loop both, and left to itself the compiler builds the second
    // table behind the fill from the first one's compare masks, kept alive across it as twelve spilled scalars
    {
        uint32_t v0 = T.c7_inc, v1 = T.c7_dec;
        asm volatile("" : "+v"(v0), "+v"(v1));
        T.c7_inc = (uint32_t)__builtin_amdgcn_readfirstlane((int)v0); T.c7_dec = (uint32_t)__builtin_amdgcn_readfirstlane((int)v1);
    }
    // What the iteration loop rebuilds a broker's band rows from (finish), four registers: per row the lookup's bias and table in the
    // small-cost form (the host picks it only for groups whose bands all fit a band_tab: search_band_tabs), the band's ends for
    // band_entry otherwise.  They are operands of per-lane arithmetic only: held in VGPRs.  The SGPR file is full and every spilled
    // scalar costs a v_readlane -- a VALU slot, the unit this kernel is bound by -- where it is used.  (The band ends themselves are
    // read again from the topic behind the loop: nothing else in it needs them.)
    constexpr bool kBandTabs = kSmall;
    int bq_r0 = kBandTabs ? band_tab_bias(T.rep_lo) : T.rep_lo, bq_r1 = kBandTabs ? (int)band_tab(T.rep_lo, T.rep_hi) : T.rep_hi;
    int bq_l0 = kBandTabs ? band_tab_bias(T.lead_lo) : T.lead_lo, bq_l1 = kBandTabs ? (int)band_tab(T.lead_lo, T.lead_hi) : T.lead_hi;
    asm volatile("" : "+v"(bq_r0), "+v"(bq_r1), "+v"(bq_l0), "+v"(bq_l1));

    // ---- LDS carve: [CUR uint4[maxP]]* [RSZ int[krt]] [XR u8[Bx rounded to 64]] then per wave
    //      [A uint4[maxP]]* [C u32[Bx rounded to 64]] [W u16[same]] [K int[krt]] [RT int[krt]]        (* only when !kGlobalA)
    //      krt = search_rack_tab(largest rack count of the launch group): the racks plus one entry for the padding marker
    const int a_bytes = kGlobalA ? 0 : prm.maxP * NW * 4;              // a restart's working words (per wave)
    const int cur_bytes = (kGlobalA || kCurG) ? 0 : prm.maxP * NW * 4;  // the topic's current-assignment words (shared by the workgroup)
    const int bx64 = (prm.maxBx + 63) & ~63;
    const int c_bytes = bx64 * 4;
    const int krt = search_rack_tab(prm.maxR);
    int *RSZ = reinterpret_cast<int *>(smem + cur_bytes);
    uint8_t *XR = smem + cur_bytes + krt * 4;  // rack of internal index x, inv = krt - 1 (never a rack) = padding slot / beyond Bx
    const uint32_t inv = (uint32_t)krt - 1u;
    uint32_t *PR = reinterpret_cast<uint32_t *>(smem + cur_bytes + krt * 4 + bx64);  // [bx64] packed prices (kPriced only)
    const bool hbw = kPriced && prm.bw != 0;   // the launch group carries broker weights (their table is carved only then)
    const int pr_bytes = kPriced ? (hbw ? 2 : 1) * c_bytes + krt * 4 : 0;
    int *PG = reinterpret_cast<int *>(smem + cur_bytes + krt * 4 + bx64 + c_bytes);  // [krt] rack prices (kPriced only)
    uint32_t *BW = reinterpret_cast<uint32_t *>(smem + cur_bytes + krt * 4 + bx64 + c_bytes + krt * 4);  // [bx64] broker weights (kPriced only)
    // per wave: [A] [C] [W] [K] [RT]; a team shares ONE [C] [W] [K], then one [RT] per wavefront and the proposal records
    unsigned char *wb = smem + cur_bytes + krt * 4 + bx64 + pr_bytes + (kTeam ? 0 : wave * (a_bytes + c_bytes + c_bytes / 2 + krt * 8));
    const Part<NW> *cur_words = reinterpret_cast<const Part<NW> *>(pl.cur_pool + TD->cur_off);  // host-prepared words x | rack << 16 (0xFFFFFFFF = none); cur_off counts words
    const Part<NW> *CUR;
    if (kGlobalA || kCurG) CUR = cur_words; else CUR = reinterpret_cast<const Part<NW> *>(smem);
    WaveLds<NW> L;
    L.C = reinterpret_cast<uint32_t *>(wb + a_bytes);
    L.W = reinterpret_cast<uint16_t *>(wb + a_bytes + c_bytes);
    L.K = reinterpret_cast<int *>(wb + a_bytes + c_bytes + c_bytes / 2);
    L.RT = L.K + krt + (kTeam ? wave * krt : 0);
    // team: proposal records, two buffers (iteration parity) x W x kTeamRec ints, then W partial sums x 2
    int *TR = L.K + krt + n_waves * krt;
    int *TS = TR + 2 * 16 * kTeamRec;

    // ---- stage the rack sizes / rack-of-index table (and, when it fits, the current-assignment words) ----
    if (!kGlobalA && !kCurG) {
        Part<NW> *cur_lds = reinterpret_cast<Part<NW> *>(smem);
        for (int p = threadIdx.x; p < T.P; p += blockDim.x) cur_lds[p] = cur_words[p];
    }
    for (int r = threadIdx.x; r < krt; r += blockDim.x) {
        RSZ[r] = r < T.R ? pl.rsz_pool[TD->rsz_off + r] : 0;
        if (kPriced) PG[r] = r < T.R ? price_units(pl.price_pool[TD->price_off + 2 * TD->B + r], prm.obj_scale) : 0;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < ((T.Bx + 63) & ~63); x += blockDim.x) {
        const uint32_t r = mulhi((uint32_t)x, T.magic);
        const bool valid = x < T.Bx && (int)((uint32_t)x - r * (uint32_t)T.m) < RSZ[r < (uint32_t)krt ? r : 0];
        XR[x] = valid ? (uint8_t)r : (uint8_t)inv;
        if (kPriced) {  // prices of broker x in key units: replica price a[b] | leader price l[b] << 16
            uint32_t pr = 0;
            if (valid) {
                const int32_t *pp = pl.price_pool + TD->price_off;
                const int b = pl.ext_pool[TD->ext_off + x];
                pr = ((uint32_t)price_units(pp[b], prm.obj_scale) & 0xFFFFu) | ((uint32_t)price_units(pp[TD->B + b], prm.obj_scale) << 16);
            }
            PR[x] = pr;
            if (hbw) BW[x] = (valid && TD->has_bw) ? pl.bw_pool[TD->bw_off + x] : 0u;
        }
    }
    __syncthreads();

    const int rho = bm.y + (kTeam ? 0 : wave);
    if (rho >= TD->n_restarts) {  // no block-level barrier below this point (a team is one restart: all or none) ...
        if constexpr (kCanChunk) chunk_pass(pc.ticket);   // ... but the hand-off's: a wavefront without a restart meets the others there
        return;
    }
    const int g = TD->restart_base + rho;
    // restart state in HBM: packed 4 x u16 per partition (LDS path, loaded / stored around the launch) or the
    // working words themselves, 16 B per partition, updated in place (global path)
    unsigned char *state_packed = pl.state_pool + TD->state_off + (uint64_t)rho * T.P * (NW * 2);
    if (kGlobalA) L.A = reinterpret_cast<Part<NW> *>(pl.state_pool + TD->state_off) + (uint64_t)rho * T.P;
    else L.A = reinterpret_cast<Part<NW> *>(wb);
    uint16_t *best = pl.best_pool + TD->best_off + (uint64_t)rho * T.P * T.RF;
    const uint16_t *ext = pl.ext_pool + TD->ext_off;
    const uint32_t slo = TD->seed_lo, shi = TD->seed_hi;
    const int S = prm.obj_scale;

    int best_obj, accepted;
    if (pc_init) {
        // surviving current replicas stay in their slots (init == 2: k_init has seeded the state and filled its holes)
        if (pc_init == 1)
        for (int p = tid; p < T.P; p += nthr) {
            Part<NW> c = CUR[p];
#pragma unroll
            for (int k = 1; k < NW; ++k)
                if (k >= T.RF) c.w[k] = kNoneW;
            L.A[p] = c;
        }
        best_obj = -1; accepted = 0;
    } else {
        best_obj = pl.restart_info[g * 4 + 0];
        accepted = pl.restart_info[g * 4 + 3];
        // (a later chunk reads what another workgroup wrote in this launch: a vector load behind chunk_take's fence, never a scalar
        //  one; the two values are wave-uniform and the loop counts `accepted` on the scalar unit)
        if constexpr (kCanChunk) { best_obj = __builtin_amdgcn_readfirstlane(best_obj); accepted = __builtin_amdgcn_readfirstlane(accepted); }
        // Elite rule: a restart whose best feasible objective trails the topic's best (as of the previous step) re-seeds
        // its state from that assignment with probability 1/2 (hash of seed, restart, launch); the elite's own restart and
        // the restarts that tie with it keep going, so the population stays diverse.
        bool reseed = false;
        if (pc_elite) {
            const unsigned long long ek = pl.elite_key[bm.x];
            const int e_obj = (int)kObjCap - (int)((ek >> 20) & 0xFFFFFFull);
            reseed = ek != ~0ull && (ek >> 44) == 0 && (int)(ek & 0xFFFFFull) != rho && best_obj < e_obj &&
                     (fmix32(slo ^ ((uint32_t)rho * 0x9E3779B1u) ^ (prm.launch * 0x85EBCA77u) ^ 0xE117Eu) & 1u);
        }
        if (reseed) {
            const uint16_t *ea = pl.elite_assign + TD->win_off;
            const uint16_t *io = pl.int_pool + TD->int_off;
            for (int p = tid; p < T.P; p += nthr) {
                Part<NW> w;
#pragma unroll
                for (int k = 0; k < NW; ++k) w.w[k] = k < T.RF ? to_word(T, io[ea[p * T.RF + k]]) : kNoneW;
                L.A[p] = w;
            }
        } else if (!kGlobalA) {
            for (int p = lane; p < T.P; p += 64) L.A[p] = load_packed<NW>(T, state_packed, p);
        }
    }
    if (kGlobalA) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // own stores visible to every lane's loads
    if (kTeam) __syncthreads();
    recount(T, L, tid, nthr, krt);
    if (kTeam) __syncthreads();

    // W from the counters: current with C from here on -- through the hole filling, which scores its candidates from it, and through every
    // accepted move of the loop below.  (A team strides it together; its first wavefront then fills the holes alone.)
    rebuild_band_state(T, L, XR, inv, tid, nthr);
    if (lane == 0) L.RT[krt - 1] = 0;                 // the spare entry padding lanes read
    if (kTeam) __syncthreads();

    if (pc_init == 1) {
        // ---- hole filling by best insertion, holes in (p,k) order, in band-state form (fill_hole, kao_search_dev.h): per listed
        //      partition its brokers are marked in W, per hole a rack table is built and every index is scored from W and RT, 64 per
        //      round; the winner's counters and band rows are brought up to date at once, so W stays what rebuild_band_state would
        //      compute, and the winner is marked before the partition's next hole is scanned. ----
        // Two passes: leader holes of all partitions first, then follower holes (leaders are the scarcer resource).
        // Round 4: the partitions that have a hole are listed by the host (TopicDev::hole_off: static, they depend on the current
        // assignment only) -- inspecting all P partitions twice, 64 per trip with a global load each, was most of the 70-ms first
        // launch of a 100,000-partition topic, holes or not.  Same holes, same order.
        // Objective weights: a candidate has one only as a current replica of the partition that is not in its working words.  RFT = 3:
        // the working words start as the current ones and the fill only adds, so no candidate has a weight and none is scored.
        // Elsewhere the current RF may exceed RF: the rounds that hold a dropped current replica are scored with weights.
        constexpr bool kFillWeights = RFT != 3;
        const uint32_t *HL = pl.cur_pool + TD->hole_off;
        const FillTabs F{L.W, XR, L.K, L.RT, PR, PG, hbw ? BW : nullptr};
        // (a team: its first wavefront fills the holes, in the same order as a single one; the others wait at the barrier behind the
        //  fill and read nothing before it, so the marks in the shared W are this wavefront's own business)
        if (!kTeam || wave == 0)
        for (int pass = 0; pass < 2; ++pass) {
            const uint32_t n_holes = HL[pass], *hl = HL + 2 + (pass ? HL[0] : 0u);
            // the next hole's rows are loaded while this one is scanned (a pass lists every partition once, so the rows of the next
            // hole cannot be written by this one): config 5 as one topic has 15,000 holes, each two global round trips apart
            int p_n = n_holes ? (int)hl[0] : 0;
            Part<NW> a_n = L.A[p_n], c_n = CUR[p_n];
            for (uint32_t hi = 0; hi < n_holes; ++hi) {
                const int p = p_n;
                Part<NW> a = a_n;  // same address in every lane: broadcast
                const Part<NW> c = c_n;
                if (hi + 1 < n_holes) { p_n = (int)hl[hi + 1]; a_n = L.A[p_n]; c_n = CUR[p_n]; }
                fill_mark<NS>(L.W, a, lane);   // (all slots empty: nothing to mark)
                // (one body for every slot, the slot a scalar: unrolled over the words it was three copies, each with scalars of its own
                //  hoisted in front of the hole loop, in a kernel whose SGPR file is full)
#pragma nounroll
                for (int k = pass; k < (pass ? T.RF : 1); ++k) {   // pass 0: the leader slot; pass 1: the follower slots
                    if ((uint32_t)__builtin_amdgcn_readfirstlane((int)sel_slot<NS>(a, k)) != kNoneW) continue;
                    const uint32_t hmix = slo ^ fmix32(shi + (uint32_t)rho * 0x9E3779B1u + (uint32_t)(p * NW + k) * 0x27D4EB2Fu + 0x5BD1E995u + prm.gen * 0x632BE5ABu);
                    // (small cost: no clamp -- a hole's cost is lam_max * dV with |dV| <= 4, inside search_small_cost's 8 lam_max + 4 S w_max)
                    const uint32_t xw_win = fill_hole<NS, kPriced, !kSmall, kFillWeights>(T, F, a, c, k == 0, hmix, prm.lam_max, S, lane);
                    if (xw_win == kNoneW) continue;   // (no candidate: fewer valid brokers than replicas, refused by the model)
                    set_slot(a, k, xw_win);
                    if (lane == 0) {
                        // the winner's counters, then its band rows from them (the replica row; the leader row too for a leader hole),
                        // written with the mark: it is a broker of the partition now
                        const uint32_t xs = xw_win & 0xFFFFu;
                        reinterpret_cast<uint32_t *>(&L.A[p])[k] = xw_win;
                        const uint32_t cx = L.C[xs] + ((k == 0) ? 0x10001u : 1u);
                        L.C[xs] = cx;
                        L.K[xw_win >> 16] += 1;
                        uint32_t wx = band_row<kBandTabs>((int)(cx & 0xFFFFu), bq_r0, bq_r1);
                        if (k == 0) wx |= band_row<kBandTabs>((int)(cx >> 16), bq_l0, bq_l1) << 6;
                        else wx |= L.W[xs] & kWRowL;
                        L.W[xs] = (uint16_t)(wx | kWNoCand);
                    }
                }
                fill_unmark<NS>(L.W, a, lane);   // the words as they are now: the winners' rows stay, without the mark
            }
        }
        if (kGlobalA) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        if (kTeam) __syncthreads();
    }

    int V, obj;
    full_cost<NW, kTeam>(T, L, CUR, RSZ, tid, nthr, V, obj, hbw ? BW : nullptr, TS, wave, n_waves);
    if (V == 0 && obj > best_obj) { best_obj = obj; snapshot(T, L, ext, best, tid, nthr); }
    if (kTeam) __syncthreads();

    // ---- per-lane RNG stream of this launch (LCG mod 2^24, re-keyed every launch) ----
    uint32_t rng = fmix32(slo ^ fmix32(shi + (uint32_t)rho * 0x9E3779B1u + prm.launch * 0x85EBCA77u + (uint32_t)tid * 0xC2B2AE3Du));   // (team: wavefront w's lanes are streams 64 w .. 64 w + 63)
    if constexpr (kCanChunk) {   // a later chunk carries the launch's streams on: the words its predecessor stored
        if (pc.later) rng = pl.chunk_rng[(size_t)g * 64 + lane];
        // The ticket waits in the wavefront's generator words, dead until the epilogue stores the next ones, and is read back behind
        // the loop: one scalar fewer live across it (every lane its own word: a plain vector store and load of the same address).
        pl.chunk_rng[(size_t)g * 64 + lane] = pc.ticket;
    }

    const int plog = TD->period_log2 + (rho & 3);
    const uint32_t pmask = (1u << plog) - 1u;
    const uint32_t lrange = (uint32_t)(prm.lam_max - prm.lam_min + 1);
    const uint32_t RF8 = (uint32_t)T.RF << 8, R8 = (uint32_t)T.R << 8, m8 = (uint32_t)T.m << 8;  // all < 65536

    const int T_tour = min(64, max(4, (T.P * T.RF) >> 2));  // lanes taking part in the slot tournament
    uint32_t tour_off = lane < T_tour ? 0u : kKeyNull;       // OR-ed into a lane's tournament key (a select would put a branch between the slots of a trip)
    asm volatile("" : "+v"(tour_off));
    const int GA = min(16, max(1, (T.P * T.RF) >> 8));       // random slots scored per lane
    const int x_rounds_full = (T.P + 63) >> 6;
    const bool x_windowed = x_rounds_full > 8;               // EXCHANGE scans at most 8 rounds of 64 partitions

    // the launch parameters the loop needs, as scalars of their own: read straight from `prm` they stay one 8-dword register
    // tuple (the kernarg load) that the allocator spills and restores WHOLE -- three times per iteration, 24 v_readlane
    int lam_lo = prm.lam_min, lam_hi = prm.lam_max;
    uint32_t n_iters = kChunked ? pc.n : prm.iters, it_base = prm.launch * prm.iters + (kChunked ? pc.first : 0u);
    // One scalar for the loop's wave-uniform choice -- bit 29: REPLACE scan over two tournament slots (topics up to kScanTwoSlots
    // replica slots) -- and, small cost, for the penalty's parameters as well: lam_min in bits 11:0, lam_max in bits 23:12
    // (0 <= lam_min <= lam_max <= 2048 by search_small_cost), the period's exponent (at most 23) in bits 28:24.  Read through an empty
    // asm where it is used: a field taken out in front of the loop is one more live scalar there, and the SGPR file is full -- each is
    // a spill restore, a v_readlane, per use.
    constexpr uint32_t kLpScanTwo = 1u << 29;
    uint32_t loop_pack = TD->P * TD->RF <= prm.scan2_max ? kLpScanTwo : 0u;
    if (kSmall) loop_pack |= ((uint32_t)prm.lam_min & 0xFFFu) | (((uint32_t)prm.lam_max & 0xFFFu) << 12) | (((uint32_t)plog & 31u) << 24);
    {   // through a VGPR and back: a plain scalar copy is coalesced with the tuple again
        uint32_t v0 = (uint32_t)lam_lo, v1 = (uint32_t)lam_hi, v2 = n_iters, v3 = it_base, v4 = loop_pack;
        asm volatile("" : "+v"(v2), "+v"(v3), "+v"(v4));
        if constexpr (!kSmall) {   // (small cost: the penalty's parameters come out of loop_pack alone)
            asm volatile("" : "+v"(v0), "+v"(v1));
            lam_lo = (int)__builtin_amdgcn_readfirstlane(v0); lam_hi = (int)__builtin_amdgcn_readfirstlane(v1);
        }
        n_iters = __builtin_amdgcn_readfirstlane(v2); it_base = __builtin_amdgcn_readfirstlane(v3);
        loop_pack = __builtin_amdgcn_readfirstlane(v4);
    }
    auto loop_flag = [&](uint32_t bit) { uint32_t lp = loop_pack; asm volatile("" : "+s"(lp)); return (lp & bit) != 0u; };
    // Fused two-slot REPLACE scan (LDS-resident, unpriced, one chunk of at most 256 rounds): slot 2's draw of round rd is the generator
    // state n_rd steps after slot 1's, s' = A_n s + C_n (mod 2^24) -- the jump-ahead of lcg24 over n_rd = rounds of the topic's scan
    constexpr bool kFuse = !kGlobalA && !kTeam && !kPriced;
    const bool fuse_ok = kFuse && T.Bx <= 16384;
    uint32_t jmp_a = 1u, jmp_c = 0u;
    if (fuse_ok)
        for (int n = (T.Bx + 63) >> 6; n > 0; --n) { jmp_a = (jmp_a * 0x6D2B79u) & 0xFFFFFFu; jmp_c = (jmp_c * 0x6D2B79u + 0x3C6EF3u) & 0xFFFFFFu; }
    // best_obj is wave-uniform and changes only at a snapshot, behind a wave-uniform branch (snapshot() loops a uniform number of
    // times for that: a lane-dependent loop bound merged with the branch and made everything set behind it a per-lane value).  Its
    // sign is "has been feasible once", what the penalty depends on: a scalar compare
    best_obj = __builtin_amdgcn_readfirstlane(best_obj);
    for (uint32_t i = 0; i < n_iters; ++i) {
        const uint32_t it = it_base + i;
        const int type = (int)((0x1210u >> ((it & 7u) * 2u)) & 3u);  // pattern R R X R L R X R
        // no oscillation before the restart has been feasible once (best_obj < 0): the penalty stays at lam_max.  Formed on the scalar
        // unit -- a scalar register is what the keys' multiply-adds take it from (mad24s, pk_mad_ss).  Small cost: its four parameters
        // come out of one packed scalar each iteration (opaque to the compiler: unpacked once in front of the loop they are four
        // more live scalars, each a spill restore -- a v_readlane -- per iteration)
        int lam;
        if constexpr (kSmall) {
            uint32_t lp = loop_pack;
            asm volatile("" : "+s"(lp));
            const uint32_t plg = (lp >> 24) & 31u;
            const int lo_ = (int)(lp & 0xFFFu), hi_ = (int)((lp >> 12) & 0xFFFu);
            const uint32_t ph = it & ((1u << plg) - 1u);
            lam = best_obj < 0 ? hi_ : min(hi_, lo_ + (int)((2u * ph * (uint32_t)(hi_ - lo_ + 1)) >> plg));
        } else {
            const uint32_t ph = it & pmask;
            lam = best_obj < 0 ? lam_hi : min(lam_hi, lam_lo + (int)((2u * ph * lrange) >> plog));
        }
        // REPLACE alternates, in blocks of 8 iterations, between "scan" (one slot, every broker) and "sample"
        // (every lane its own slot, 4 brokers); EXCHANGE always scans; LEADER-SWAP always samples
        const bool sampled = (type == 2) || (type == 0 && ((it >> 3) & 1u));

        // ---- from a kind's winning proposal to the applied move.  Every move kind below keeps its per-lane proposal (key, p, k, uw, vw,
        //      dV, dObj; an EXCHANGE also q, j) in its own scope and ends here, with the kind as a compile-time constant: a REPLACE never
        //      touches q / j, a LEADER-SWAP always rebuilds the leader row, and no proposal variable is shared -- and copied at the
        //      joins -- between the kinds.  `ty`: 0 REPLACE, 1 EXCHANGE, 2 LEADER-SWAP (= the wave-uniform `type`).  `uni`: the proposal
        //      is wave-uniform (both REPLACE scans recompute the winner's move in every lane), so nothing is read from lane `win`. ----
        auto finish = [&](auto ty, auto uni, uint32_t kmin, int win, int p, int k, int q, int j, uint32_t uw, uint32_t vw, int dV, int dObj) {
            constexpr int TY = decltype(ty)::value;
            auto of_win = [&](int v) { return decltype(uni)::value ? v : __builtin_amdgcn_readlane(v, win); };
            if (!kTeam) {
                if (kmin == kKeyNull) return;
                if ((int)(kmin >> 8) - kDBias > 0) return;  // accept only non-worsening moves (cost under current lam)
            }
            bool mine = true;   // team: this wavefront's proposal is applied
            int *rec = TR + ((i & 1u) * 16 + (uint32_t)wave) * kTeamRec;
            if (kTeam) {
                // ---- the team's proposals meet: record = {acceptable, p, q, broker out, broker in, rack out, rack in, dV, dObj, applied} ----
                const bool ok = kmin != kKeyNull && (int)(kmin >> 8) - kDBias <= 0;
                if (lane == win) {
                    const uint32_t ro_ = uw >> 16, rn_ = vw >> 16;
                    const bool racks = ok && TY == 0 && ro_ != rn_;   // only a REPLACE across racks reads and changes rack totals
                    rec[0] = ok ? 1 : 0; rec[1] = p; rec[2] = TY == 1 ? q : p;
                    rec[3] = (int)(uw & 0xFFFFu); rec[4] = (int)(vw & 0xFFFFu);
                    rec[5] = racks ? (int)ro_ : 0xFFFF; rec[6] = racks ? (int)rn_ : 0xFFFF;
                    rec[7] = dV; rec[8] = dObj;
                }
                __syncthreads();
                bool clash = false;
                if (lane < wave) {   // lane l looks at wavefront l's record: only lower-numbered wavefronts can block this one
                    const int *o = TR + ((i & 1u) * 16 + (uint32_t)lane) * kTeamRec;
                    if (o[0]) {
                        const int mp = rec[1], mq = rec[2], mb0 = rec[3], mb1 = rec[4], mr0 = rec[5], mr1 = rec[6];
                        clash = (o[1] == mp) | (o[1] == mq) | (o[2] == mp) | (o[2] == mq) | (o[3] == mb0) | (o[3] == mb1) | (o[4] == mb0) | (o[4] == mb1);
                        if (o[5] != 0xFFFF && mr0 != 0xFFFF) clash |= (o[5] == mr0) | (o[5] == mr1) | (o[6] == mr0) | (o[6] == mr1);
                    }
                }
                mine = ok && __ballot(clash) == 0ull;
            }

            // The small-cost instantiations take the one-trip form below.  The others keep the form a team needs: with the one-trip form
            // k_search<0,0,4,1,3,0> and <0,0,4,0,0,0> spilled a vector register to scratch (8 B, docs/notes_r15.md section 1).
            constexpr bool kOneTrip = !kTeam && kSmall;
            if constexpr (kOneTrip) {
                // ---- one wavefront, one restart.  The winning lane writes the partition words.  The counters the move changes -- the two
                //      brokers' words of C and, for a REPLACE across racks, the two racks' totals in K -- are each owned by one of lanes
                //      0..3: lane 0 the old broker, lane 1 the new one, lane 2 the old rack, lane 3 the new one.  All read together and
                //      write together, and lanes 0 / 1 read their broker's band-state word along with its counter and rebuild its rows
                //      from the counter value they have just formed: ONE dependent LDS round trip where four read-modify-writes behind
                //      one another (the compiler cannot tell that the addresses differ), a second read of C and one of W took six.
                //      Old and new broker always differ (a partition's own brokers are no candidates, the two slots of an EXCHANGE or a
                //      LEADER-SWAP hold different brokers); a REPLACE inside one rack leaves its total alone: lanes 2 / 3 sit out. ----
                if (lane == win) {
                    uint32_t *ap = reinterpret_cast<uint32_t *>(&L.A[p]);
                    if (TY == 0) ap[k] = vw;
                    else if (TY == 1) { ap[k] = vw; reinterpret_cast<uint32_t *>(&L.A[q])[j] = uw; }
                    else { ap[0] = vw; ap[k] = uw; }
                }
                // Which rows move: a REPLACE of a follower slot moves the replica counts (row C3), a LEADER-SWAP and an EXCHANGE between a
                // leader and a follower slot the leader counts (row C4), a REPLACE of a leader slot both, an EXCHANGE between two slots of
                // one kind no count at all.  The kind of the move is wave-uniform: the winner's slot numbers.  Only the row whose count
                // moved is rebuilt and inserted into the broker's word (the scan's marks have been restored by now and a padding index
                // is never accepted, so bits 15:12 are zero either way).
                const int kw = of_win(k);
                int rows;   // bit 0: the replica row, bit 1: the leader row
                if (TY == 0) rows = 1 | (kw == 0 ? 2 : 0);
                else if (TY == 1) rows = (kw == 0 ? 2 : 0) ^ (of_win(j) == 0 ? 2 : 0);
                else rows = 2;
                if (rows != 0) {
                    // (the winner's two words as scalars: a uniform proposal holds the new one in a vector register, the same in every lane)
                    const uint32_t uws = (uint32_t)of_win((int)uw);
                    const uint32_t vws = decltype(uni)::value ? (uint32_t)__builtin_amdgcn_readfirstlane((int)vw) : (uint32_t)of_win((int)vw);
                    const uint32_t xo = uws & 0xFFFFu, xn = vws & 0xFFFFu;
                    uint32_t xx = xo;   // the broker a lane reads W of (lanes 2 / 3: the old broker's, a value they drop)
                    asm("v_writelane_b32 %0, %1, 1" : "+v"(xx) : "s"(xn));
                    uint32_t xi = xx;   // the entry a lane owns: an index of C (lanes 0 / 1) or of K (lanes 2 / 3)
                    // what the old broker's word loses (the new one's gains): a replica, with the leader when the slot is the leader's; an
                    // EXCHANGE moves the leader from u to v (k the leader slot) or from v to u
                    const uint32_t d0 = TY == 0 ? (kw == 0 ? 0x10001u : 1u) : (TY == 1 ? (kw == 0 ? 0x10000u : 0u - 0x10000u) : 0x10000u);
                    int n_own = 2;
                    if (TY == 0) {
                        const uint32_t ro_ = uws >> 16, rn_ = vws >> 16;
                        asm("v_writelane_b32 %0, %1, 2\n\tv_writelane_b32 %0, %2, 3" : "+v"(xi) : "s"(ro_), "s"(rn_));
                        n_own = ro_ != rn_ ? 4 : 2;
                    }
                    int lane_w = lane;   // (through an empty asm: the masks are compares here, not spilled scalar pairs hoisted out of the loop)
                    asm volatile("" : "+v"(lane_w));
                    if (lane_w < n_own) {
                        uint32_t *cp = (lane_w < 2 ? L.C : reinterpret_cast<uint32_t *>(L.K)) + xi;
                        const uint32_t c_old = *cp;
                        const uint32_t w_old = L.W[xx];
                        const uint32_t dl = lane_w < 2 ? d0 : 1u;
                        const uint32_t cx = (lane_w & 1) ? c_old + dl : c_old - dl;
                        *cp = cx;
                        if (lane_w < 2) {
                            uint32_t wx;
                            if (rows == 3) wx = band_row<kBandTabs>((int)(cx & 0xFFFFu), bq_r0, bq_r1) | (band_row<kBandTabs>((int)(cx >> 16), bq_l0, bq_l1) << 6);
                            else if (rows == 1) wx = (w_old & ~kWRowR) | band_row<kBandTabs>((int)(cx & 0xFFFFu), bq_r0, bq_r1);
                            else wx = (w_old & ~kWRowL) | (band_row<kBandTabs>((int)(cx >> 16), bq_l0, bq_l1) << 6);
                            L.W[xx] = (uint16_t)wx;
                        }
                    }
                }
            } else {
            if (lane == win && mine) {  // the winning lane applies its own proposal
                uint32_t *ap = reinterpret_cast<uint32_t *>(&L.A[p]);
                if (TY == 0) {
                    const uint32_t d = (k == 0) ? 0x10001u : 1u;
                    L.C[uw & 0xFFFFu] -= d;
                    L.C[vw & 0xFFFFu] += d;
                    if (!kTeam || (uw >> 16) != (vw >> 16)) {   // (team: moves inside one rack do not own its total -- two of them may run at once)
                        L.K[uw >> 16] -= 1;
                        L.K[vw >> 16] += 1;
                    }
                    ap[k] = vw;
                } else if (TY == 1) {
                    uint32_t *bp = reinterpret_cast<uint32_t *>(&L.A[q]);
                    if ((k == 0) != (j == 0)) {
                        const uint32_t lose = (k == 0) ? uw : vw, gain = (k == 0) ? vw : uw;
                        L.C[lose & 0xFFFFu] -= 0x10000u;
                        L.C[gain & 0xFFFFu] += 0x10000u;
                    }
                    ap[k] = vw;
                    bp[j] = uw;
                } else {
                    L.C[uw & 0xFFFFu] -= 0x10000u;
                    L.C[vw & 0xFFFFu] += 0x10000u;
                    ap[0] = vw;
                    ap[k] = uw;
                }
            }
            if (mine) {   // band state of the two brokers whose counters have changed: lane 0 the old broker, lane 1 the new one
                // Only the row whose count moved is rebuilt and inserted into the broker's word (the scan's marks have been restored by
                // now and a padding index is never accepted, so bits 15:12 are zero either way): a REPLACE of a follower slot moves the
                // replica counts (row C3), a LEADER-SWAP and an EXCHANGE between a leader and a follower slot the leader counts (row
                // C4), a REPLACE of a leader slot both, an EXCHANGE between two slots of one kind no count at all.  The kind of the
                // move is wave-uniform: the winner's slot numbers.
                int rows;   // bit 0: the replica row, bit 1: the leader row
                if (TY == 0) rows = 1 | (of_win(k) == 0 ? 2 : 0);
                else if (TY == 1) rows = (of_win(k) == 0 ? 2 : 0) ^ (of_win(j) == 0 ? 2 : 0);
                else rows = 2;
                if (rows != 0) {
                    // (a uniform proposal: masked first, the new broker's index is then the scalar the scan's winner was located by)
                    const uint32_t xo = (uint32_t)of_win((int)uw) & 0xFFFFu, xn = decltype(uni)::value ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(vw & 0xFFFFu)) : (uint32_t)of_win((int)vw) & 0xFFFFu;
                    uint32_t xx = xo;
                    asm("v_writelane_b32 %0, %1, 1" : "+v"(xx) : "s"(xn));   // lane 1: the new broker
                    int lane_w = lane;   // (through an empty asm: the mask `lane < 2` is one compare here, not a spilled scalar pair hoisted out of the loop)
                    asm volatile("" : "+v"(lane_w));
                    if (lane_w < 2) {
                        const uint32_t cx = L.C[xx];
                        uint32_t wx;
                        if (rows == 3) wx = band_row<kBandTabs>((int)(cx & 0xFFFFu), bq_r0, bq_r1) | (band_row<kBandTabs>((int)(cx >> 16), bq_l0, bq_l1) << 6);
                        else if (rows == 1) wx = (L.W[xx] & ~kWRowR) | band_row<kBandTabs>((int)(cx & 0xFFFFu), bq_r0, bq_r1);
                        else wx = (L.W[xx] & ~kWRowL) | (band_row<kBandTabs>((int)(cx >> 16), bq_l0, bq_l1) << 6);
                        L.W[xx] = (uint16_t)wx;
                    }
                }
            }
            }   // (!kOneTrip; a team: the form its record exchange orders)
            if (kGlobalA) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the winner's stores before the next loads
            if (kTeam) {
                if (lane == 0) rec[9] = mine ? 1 : 0;
                __syncthreads();
                int dVs = 0, dOs = 0, na = 0;
                if (lane < n_waves) {
                    const int *o = TR + ((i & 1u) * 16 + (uint32_t)lane) * kTeamRec;
                    if (o[9]) { dVs = o[7]; dOs = o[8]; na = 1; }
                }
                V += wave_sum(dVs);
                obj += wave_sum(dOs);
                accepted += wave_sum(na);
            } else {
                V += of_win(dV);
                obj += of_win(dObj);
                accepted++;
            }
        };
        constexpr std::integral_constant<int, 0> kReplace{};
        constexpr std::integral_constant<int, 1> kExchange{};
        constexpr std::integral_constant<int, 2> kLeaderSwap{};

        // Every violation delta of the broker rows (C3, C4) below comes from the brokers' band state W (band_fields): a signed
        // 2-bit field per (row, direction) instead of two compares, a select and a subtract on the counter word; the prices
        // of the priced instantiation apply where the matching "count leaves / re-enters its band" flag is set.
        if (sampled) {
            const int p = (int)rnd24_wide(rng, (uint32_t)T.P);
            const Part<NW> a = L.A[p];
            const Part<NW> c = CUR[p];
            uint32_t key = kKeyNull, vw = 0;   // this lane's best proposal of the iteration
            int dV = 0, dObj = 0;
            if (type == 0) {  // REPLACE (p,k) <- x_g: 2 candidates of any rack, 2 of the old broker's rack
                const int k = (int)rnd24(rng, RF8);
                const uint32_t uw = sel_slot<NS>(a, k);
                const uint32_t ro = uw >> 16;
                const bool lead = k == 0;
                const uint32_t lw = lead ? 2u : 0u;   // width of a leader field: a zero-width extract yields 0 for follower slots
                const int wl = lead ? T.w00 : T.w01, wf = lead ? T.w10 : T.w11;
                const int g_old = role_w2<NS>(c, uw, wl, wf) + (hbw ? bw_of(BW[uw & 0xFFFFu], lead) : 0);
                const uint32_t wo = L.W[uw & 0xFFFFu];
                const int dV_old = wfld(wo, kWDecR) + wfldw(wo, kWDecL, lw);
                const int dV_rack_old = ddec(L.K[ro], T.rack_lo, T.rack_hi) + c7_delta(T.c7_dec, cnt4x2<NS>(a, ro));
                const int rsz_ro = RSZ[ro];
                int dP_old = 0, dP_rack_old = 0;
                if (kPriced) {
                    const uint32_t pro = PR[uw & 0xFFFFu];
                    dP_old = -(wflag(wo, kWPoutR) & price_rep(pro));
                    if (lead) dP_old -= wflag(wo, kWPoutL) & price_lead(pro);
                    dP_rack_old = p_out(L.K[ro], T.rack_lo, T.rack_hi, PG[ro]);
                }
                // (small cost: cost + bias = lam * dV + (S * g_old + bias) - S * weight of the candidate; the winner's dObj from its weight)
                const int base_s = kSmall ? mad24s(S, g_old, kDBias) : 0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint32_t r, jj;
                    bool okg;
                    if (g < 2) {
                        r = rnd24(rng, R8);
                        jj = rnd24(rng, m8);
                        okg = (int)jj < RSZ[r];
                    } else {
                        r = ro;
                        jj = rnd24(rng, (uint32_t)rsz_ro << 8);
                        okg = true;
                    }
                    const uint32_t x = __umul24(r, (uint32_t)T.m) + jj;
                    const uint32_t xw = x | (r << 16);
                    okg = okg && !in4<NS>(a, xw);
                    const uint32_t wn = L.W[x];
                    int dVg = dV_old + wfld(wn, kWIncR) + wfldw(wn, kWIncL, lw);
                    if (g < 2) {
                        if (r != ro)
                            dVg += dV_rack_old + dinc(L.K[r], T.rack_lo, T.rack_hi) + c7_delta(T.c7_inc, cnt4x2<NS>(a, r));
                    }
                    const int dObjg = role_w2<NS>(c, xw, wl, wf) + (hbw ? bw_of(BW[x], lead) : 0) - (kSmall ? 0 : g_old);
                    uint32_t keyg;
                    if constexpr (kSmall) keyg = okg ? key_small(mad24s(-S, dObjg, mad24s(lam, dVg, base_s)), (uint32_t)lane) : kKeyNull;
                    else if (kPriced) {
                        const uint32_t prx = PR[x];
                        int dPg = dP_old + (wflag(wn, kWPinR) & price_rep(prx));
                        if (lead) dPg += wflag(wn, kWPinL) & price_lead(prx);
                        if (g < 2 && r != ro) dPg += dP_rack_old + p_in(L.K[r], T.rack_lo, T.rack_hi, PG[r]);
                        keyg = okg ? make_key_p(lam, S, dVg, dObjg, dPg, lane) : kKeyNull;
                    }
                    else keyg = okg ? make_key(lam, S, dVg, dObjg, lane) : kKeyNull;
                    if (keyg < key) { key = keyg; vw = xw; dV = dVg; dObj = dObjg; }
                }
                if constexpr (kSmall) dObj -= g_old;
                const uint32_t kmin = wave_umin(key);  // wavefront min-scan over the lanes' best proposals
                finish(kReplace, std::false_type{}, kmin, (int)(kmin & 63u), p, k, 0, 0, uw, vw, dV, dObj);
            } else {  // LEADER SWAP inside p: slot 0 <-> slot k, every k = 1..RF-1 is a candidate
                const uint32_t uw = a.w[0];
                int k = 0;
                const int u_lead = role_w2<NS>(c, uw, T.w00, T.w10), u_fol = role_w2<NS>(c, uw, T.w01, T.w11);
                const uint32_t wu = L.W[uw & 0xFFFFu];
                const int dV_u = wfld(wu, kWDecL);
                const int dP_u = kPriced ? -(wflag(wu, kWPoutL) & price_lead(PR[uw & 0xFFFFu])) : 0;
#pragma unroll
                for (int kk = 1; kk < NS; ++kk) {
                    if (!RFT && kk >= T.RF) break;
                    const uint32_t xw = a.w[kk];
                    const int dObjg = role_w2<NS>(c, xw, T.w00, T.w10) + u_fol - u_lead - role_w2<NS>(c, xw, T.w01, T.w11) +
                                      (hbw ? (int)(BW[xw & 0xFFFFu] >> 16) - (int)(BW[uw & 0xFFFFu] >> 16) : 0);
                    const uint32_t wx = L.W[xw & 0xFFFFu];
                    const int dVg = dV_u + wfld(wx, kWIncL);
                    uint32_t keyg;
                    if constexpr (kSmall) keyg = key_small(mad24s(lam, dVg, mad24s(-S, dObjg, kDBias)), (uint32_t)lane);
                    else if (kPriced) keyg = make_key_p(lam, S, dVg, dObjg, dP_u + (wflag(wx, kWPinL) & price_lead(PR[xw & 0xFFFFu])), lane);
                    else keyg = make_key(lam, S, dVg, dObjg, lane);
                    if (keyg < key) { key = keyg; vw = xw; k = kk; dV = dVg; dObj = dObjg; }
                }
                const uint32_t kmin = wave_umin(key);
                finish(kLeaderSwap, std::false_type{}, kmin, (int)(kmin & 63u), p, k, 0, 0, uw, vw, dV, dObj);
            }
        } else {
            // ---- phase A: tournament over T_tour random slots; lowest removal score wins the iteration ----
            // Score one random slot: the cost of taking its replica out under the current penalty.  REPLACE: the replica
            // leaves its broker and (at best) its rack.  EXCHANGE: broker and rack totals do not change; only the
            // partition's own rack spread (C7) and who leads (a leader slot may shed a leader, a follower slot may
            // gain one) can improve.  `type` is wave-uniform, so only one branch is ever executed.
            uint32_t keyA, oldw_l;
            int pl_, kl_, g_old_l, dvo_l = 0, dvr_l = 0;
            // `ty` is the (wave-uniform) move type as a compile-time constant: each instantiation is straight-line code, so the
            // two slots of a trip below interleave -- a big topic runs one wavefront per SIMD and the LDS round trips of one
            // slot (A[p], then W[x] / K[rack]) are hidden behind the other slot's, not behind other wavefronts
            // (p_o comes in: the lane's first slot is in a random partition, its further slots in the partitions that follow it
            //  cyclically -- on topics that live in HBM the slots of a lane then share two cache lines instead of touching 16)
            auto score_words = [&](auto ty, uint32_t &key_o, const Part<NW> &al, const Part<NW> &cl, int k_o, uint32_t &oldw_o, int &g_o, int &dvo_o, int &dvr_o) {
                constexpr int TY = decltype(ty)::value;
                oldw_o = sel_slot<NS>(al, k_o);
                const uint32_t rol = oldw_o >> 16;
                const bool leadl = k_o == 0;
                g_o = role_w2<NS>(cl, oldw_o, leadl ? T.w00 : T.w01, leadl ? T.w10 : T.w11);
                if (hbw && TY == 0) g_o += bw_of(BW[oldw_o & 0xFFFFu], leadl);   // a REPLACE also gives up the broker's own weight
                const uint32_t wo = L.W[oldw_o & 0xFFFFu];
                const int dv7 = c7_delta(T.c7_dec, cnt4x2<NS>(al, rol));
                int sc;
                if (TY == 0) {
                    dvo_o = wfld(wo, kWDecR) + wfldw(wo, kWDecL, leadl ? 2u : 0u);
                    dvr_o = ddec(L.K[rol], T.rack_lo, T.rack_hi) + dv7;
                    sc = dvo_o + min(dvr_o, 0);
                } else {
                    const int dvl = wfld(wo, leadl ? kWDecL : kWIncL);
                    sc = min(dv7, 0) + min(dvl, 0);
                }
                if constexpr (kSmall) key_o = key_small(mad24s(lam, sc, mad24s(S, g_o, kDBias)), (uint32_t)lane) | tour_off;
                else if (kPriced) {
                    int dPs = 0;
                    if (TY == 0) {
                        const uint32_t pro = PR[oldw_o & 0xFFFFu];
                        dPs = -(wflag(wo, kWPoutR) & price_rep(pro));
                        dPs -= wflagw(wo, kWPoutL, leadl ? 1u : 0u) & price_lead(pro);
                    }
                    key_o = make_key_p(lam, S, sc, -g_o, dPs, lane) | tour_off;
                }
                else key_o = make_key(lam, S, sc, -g_o, lane) | tour_off;   // lanes outside the tournament: all ones = kKeyNull
            };
            auto score_slot = [&](auto ty, uint32_t &key_o, int p_o, int &k_o, uint32_t &oldw_o, int &g_o, int &dvo_o, int &dvr_o) {
                k_o = (int)rnd24(rng, RF8);
                const Part<NW> al = L.A[p_o];
                const Part<NW> cl = CUR[p_o];
                score_words(ty, key_o, al, cl, k_o, oldw_o, g_o, dvo_o, dvr_o);
            };
            // large topics: up to 16 slots per lane, the lane keeps its best; two slots per trip.  Draw and comparison order
            // are those of a one-at-a-time loop.
            auto tournament = [&](auto ty) {
                const int p0 = (int)rnd24_wide(rng, (uint32_t)T.P);
                auto part = [&](int ga) { const int q2 = p0 + ga; return q2 < T.P ? q2 : q2 - T.P; };   // GA <= 16 <= P whenever GA > 1
                pl_ = p0;
                score_slot(ty, keyA, p0, kl_, oldw_l, g_old_l, dvo_l, dvr_l);
                int ga = 1;
                for (; kWide && ga + 1 < GA; ga += 2) {
                    uint32_t kg0, ow0, kg1, ow1;
                    int kk0, gg0, d10 = 0, d20 = 0, kk1, gg1, d11 = 0, d21 = 0;
                    const int pg0 = part(ga), pg1 = part(ga + 1);
                    score_slot(ty, kg0, pg0, kk0, ow0, gg0, d10, d20);
                    score_slot(ty, kg1, pg1, kk1, ow1, gg1, d11, d21);
                    if (kg0 < keyA) { keyA = kg0; pl_ = pg0; kl_ = kk0; oldw_l = ow0; g_old_l = gg0; dvo_l = d10; dvr_l = d20; }
                    if (kg1 < keyA) { keyA = kg1; pl_ = pg1; kl_ = kk1; oldw_l = ow1; g_old_l = gg1; dvo_l = d11; dvr_l = d21; }
                }
                for (; ga < GA; ++ga) {
                    uint32_t kg, ow;
                    int kk, gg, d1 = 0, d2 = 0;
                    const int pg = part(ga);
                    score_slot(ty, kg, pg, kk, ow, gg, d1, d2);
                    if (kg < keyA) { keyA = kg; pl_ = pg; kl_ = kk; oldw_l = ow; g_old_l = gg; dvo_l = d1; dvr_l = d2; }
                }
            };
            // Topics that live in global memory (round 4): every draw of the iteration is independent of what is loaded, so all
            // of them come first, then ALL the loads of the iteration -- the 2 x 16 tournament words of the lane and, for an
            // EXCHANGE, the partner words of the first XB rounds -- are issued back to back, and only then scored: one global round
            // trip per iteration where the slot-by-slot form took 8 for the tournament, one more for the winner's words and one per
            // partner round (a restart is one wavefront per SIMD: nothing else hides that latency).  The lane's 16 loads of
            // consecutive partitions also hit the same two or three cache lines while they are still in the L1.  Draw and
            // comparison order are those of the slot-by-slot loop (same spec, same replay); slots g >= GA of a small topic are
            // loaded from the lane's first partition and masked out of the comparison.
            Part<NW> a_l, c_l;   // the words of the lane's best slot: the winner's are broadcast, not re-read
            constexpr int XB = !kGlobalA ? 1 : ((NW == 4 && !kTeam) ? 8 : 4);   // (a team runs two wavefronts per SIMD: 256 registers each)
            Part<NW> xb[XB], xcb[XB];
            int q0 = 0;
            auto x_partner = [&](int rd, int &qq, bool &okq) {   // partition lane `lane` looks at in partner round rd
                qq = q0 + rd * 64 + lane; okq = true;
                if (qq >= T.P) { if (x_windowed) qq -= T.P; else okq = false; }
                return min(qq, T.P - 1);
            };
            auto tournament_global = [&](auto ty) {
                constexpr int TY = decltype(ty)::value;
                constexpr int TB = (NW == 4 && !kTeam) ? 16 : 8;   // slots per batch: 2 x NW x TB registers of loads in flight
                const int p0 = (int)rnd24_wide(rng, (uint32_t)T.P);
                auto part = [&](int ga) { const int q2 = p0 + ga; return q2 < T.P ? q2 : q2 - T.P; };
                int kk[16];
#pragma unroll
                for (int g = 0; g < 16; ++g) { kk[g] = 0; if (g < GA) kk[g] = (int)rnd24(rng, RF8); }
                if (TY == 1) {
                    const int q_draw = (int)rnd24_wide(rng, (uint32_t)T.P);   // every lane draws; lane 0's value places the window
                    q0 = x_windowed ? __builtin_amdgcn_readfirstlane(q_draw) : 0;
#pragma unroll
                    for (int r2 = 0; r2 < XB; ++r2) { int qq; bool okq; const int qc = x_partner(r2, qq, okq); xb[r2] = L.A[qc]; xcb[r2] = CUR[qc]; }
                }
#pragma unroll
                for (int g0 = 0; g0 < 16; g0 += TB) {
                    if (g0 > 0 && g0 >= GA) break;   // wave-uniform
                    Part<NW> tal[TB], tcl[TB];
                    int tp[TB];
#pragma unroll
                    for (int g = 0; g < TB; ++g) { tp[g] = (g0 + g) < GA ? part(g0 + g) : p0; tal[g] = L.A[tp[g]]; tcl[g] = CUR[tp[g]]; }
#pragma unroll
                    for (int g = 0; g < TB; ++g) {
                        uint32_t kg, ow;
                        int gg, d1 = 0, d2 = 0;
                        score_words(ty, kg, tal[g], tcl[g], kk[g0 + g], ow, gg, d1, d2);
                        if (g0 + g > 0) kg |= (g0 + g) < GA ? 0u : kKeyNull;
                        if (g0 + g == 0 || kg < keyA) { keyA = kg; pl_ = tp[g]; kl_ = kk[g0 + g]; oldw_l = ow; g_old_l = gg; dvo_l = d1; dvr_l = d2; a_l = tal[g]; c_l = tcl[g]; }
                    }
                }
            };
            if constexpr (kGlobalA) { if (type == 0) tournament_global(std::integral_constant<int, 0>{}); else tournament_global(std::integral_constant<int, 1>{}); }
            else if (type == 0) tournament(std::integral_constant<int, 0>{}); else tournament(std::integral_constant<int, 1>{});
            const int wA1 = (int)(wave_umin(keyA) & 63u);
            // REPLACE scan (round 4): the slots of the tournament's TWO best lanes are scanned, the winner's first; the better of
            // the two moves is the proposal (ties: the first slot's).  Loop head, penalty, acceptance and bookkeeping are paid once
            // for twice the neighbours (they were two thirds of the instruction stream at 500 brokers, docs/notes_r03.md section 6).
            int wA2 = -1;
            if (type == 0 && loop_flag(kLpScanTwo)) {   // (large topics scan one slot: their iterations are what they are short of)
                const uint32_t k2 = wave_umin(lane == wA1 ? kKeyNull : keyA);
                wA2 = k2 == kKeyNull ? -1 : (int)(k2 & 63u);   // (no other lane takes part: one slot)
            }
            if (kFuse && type == 0 && wA2 >= 0 && fuse_ok) {
                // ---- phase B (REPLACE), both tournament slots in ONE pass over the brokers (round 7).  The two slots score the same
                //      brokers from the same W / XR words: each round loads them once and forms both slots' keys, two running minima.
                //      Per slot everything is as in the one-slot scan below: its own RT half (the rack part of the delta, packed in the
                //      two 16-bit halves of RT), its own no-candidate bit in W (slot 1: bit 15, slot 2: bit 14), its own weighted rounds
                //      (the union of both slots' rounds is scored with weights: a slot's weights are zero on brokers outside its
                //      current replicas), its own draw sequence (slot 2's round rd: jump-ahead of slot 1's draw by n_rd steps).  The
                //      move is that of the slot with the strictly lower wave minimum (ties: slot 1), recomputed once.
                int ps[2], ks[2], gs[2], dvos[2];
                uint32_t us[2];
                int v_rk[2];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const int wA = s2 == 0 ? wA1 : wA2;
                    ps[s2] = __builtin_amdgcn_readlane(pl_, wA);
                    ks[s2] = __builtin_amdgcn_readlane(kl_, wA);
                    us[s2] = (uint32_t)__builtin_amdgcn_readlane((int)oldw_l, wA);
                    gs[s2] = __builtin_amdgcn_readlane(g_old_l, wA);
                    dvos[s2] = __builtin_amdgcn_readlane(dvo_l, wA);
                    v_rk[s2] = __builtin_amdgcn_readlane(dvr_l, wA);
                }
                const Part<NW> a1 = L.A[ps[0]], c1 = CUR[ps[0]], a2 = L.A[ps[1]], c2 = CUR[ps[1]];
                const uint32_t ro1 = us[0] >> 16, ro2 = us[1] >> 16;
                for (int r = lane; r < T.R; r += 64) {
                    const int dk = dinc(L.K[r], T.rack_lo, T.rack_hi);
                    const int v1 = ((uint32_t)r != ro1) ? v_rk[0] + dk + c7_delta(T.c7_inc, cnt4x2<NS>(a1, (uint32_t)r)) : 0;
                    const int v2 = ((uint32_t)r != ro2) ? v_rk[1] + dk + c7_delta(T.c7_inc, cnt4x2<NS>(a2, (uint32_t)r)) : 0;
                    // (small cost: slot 1 rides in the HIGH half -- its no-candidate mark, bit 15 of W, is the upper half of the sign-extended word)
                    L.RT[r] = kSmall ? (int)(((uint32_t)v2 & 0xFFFFu) | ((uint32_t)v1 << 16)) : (int)(((uint32_t)v1 & 0xFFFFu) | ((uint32_t)v2 << 16));
                }
                // lanes 0..NW-1 look after slot 1's partition, lanes NW..2NW-1 after slot 2's: their brokers are marked, their
                // displaced current replicas listed.  (Each lane reads its own word.  The lane number goes through an empty asm: the
                // lane masks derived from it are then one compare each here; hoisted out of the iteration loop they were spilled
                // scalar pairs, two v_readlane restores per use.)
                int lane_v = lane;
                asm volatile("" : "+v"(lane_v));
                const int li = lane_v & (NW - 1);
                const bool l2 = lane_v >= NW;
                const int p_l = l2 ? ps[1] : ps[0];
                const uint32_t ai = reinterpret_cast<const uint32_t *>(&L.A[p_l])[li], ci = reinterpret_cast<const uint32_t *>(&CUR[p_l])[li];
                const bool holds = (lane_v < 2 * NW) & (ai != kNoneW);
                // (slot 1's lanes mark first, then slot 2's lanes read the word again and add their bit: a broker in both partitions
                //  carries both bits without comparing every broker against the other partition's words; the restore writes the
                //  word read before either mark, the same value from both lanes.  A current replica is in its slot's partition
                //  exactly when the marks gave it that slot's bit.)
                uint32_t w_keep = 0;
                if (holds) w_keep = L.W[ai & 0xFFFFu];
                if (holds & !l2) L.W[ai & 0xFFFFu] = (uint16_t)(w_keep | kWNoCand);
                if (holds & l2) L.W[ai & 0xFFFFu] = (uint16_t)(L.W[ai & 0xFFFFu] | kWNoCand2);
                const bool hc = (lane_v < 2 * NW) & (ci != kNoneW);
                uint32_t w_ci = 0;
                if (hc) w_ci = L.W[ci & 0xFFFFu];
                const bool hm_l = hc & ((w_ci & (l2 ? kWNoCand2 : kWNoCand)) == 0u);
                const int mr_l = hm_l ? (int)((ci & 0xFFFFu) >> 6) : -1;
                int mr[2 * NW];
#pragma unroll
                for (int i2 = 0; i2 < 2 * NW; ++i2) mr[i2] = (i2 & (NW - 1)) < NS ? __builtin_amdgcn_readlane(mr_l, i2) : -1;   // (RFT: lanes 3 / 7 hold none)
                const bool lead1 = ks[0] == 0, lead2 = ks[1] == 0;
                const uint32_t lw1 = lead1 ? 2u : 0u, lw2 = lead2 ? 2u : 0u;
                const int wl1 = lead1 ? T.w00 : T.w01, wf1 = lead1 ? T.w10 : T.w11, wl2 = lead2 ? T.w00 : T.w01, wf2 = lead2 ? T.w10 : T.w11;
                const int K01 = __mul24(S, gs[0]) + kDBias + __mul24(lam, dvos[0]);
                const int K02 = __mul24(S, gs[1]) + kDBias + __mul24(lam, dvos[1]);
                // small cost: both slots' costs in the int16 halves of one register, slot 1 high / slot 2 low.  The bias stays inside K0: the
                // low 16 bits of a product-sum are the same signed and unsigned, so each half IS that slot's cost field.  The weights of a
                // weighted round are scaled once, each in its slot's half.
                const uint32_t leadp = (lead2 ? 1u : 0u) | (lead1 ? 0x10000u : 0u);
                const uint32_t K0p = ((uint32_t)K02 & 0xFFFFu) | ((uint32_t)K01 << 16);
                const int wl1h = (int)((uint32_t)(S * wl1) << 16), wf1h = (int)((uint32_t)(S * wf1) << 16);
                const int wl2s = (int)((uint32_t)(S * wl2) & 0xFFFFu), wf2s = (int)((uint32_t)(S * wf2) & 0xFFFFu);
                uint32_t jc = jmp_c;
                asm volatile("" : "+v"(jc));
                uint32_t best1 = kKeyNull, best2 = kKeyNull;   // (cost + bias) << 16 | tie << 8 | round, per slot
                // A round is its loads -- W (one ds_read_i16: sign-extended, bit 15 fills the upper half) and XR of the lane's index, then RT
                // of that rack -- and its arithmetic (scan_round2).  The rounds of a scan do not depend on each other, but a wavefront
                // waits for every LDS round trip it has started before it uses one: a trip of two rounds issues its four W / XR reads
                // together and its two RT reads together, two dependent trips where round after round took four.  Only indices of
                // rounds the scan scores anyway are read.
                const short *Ws = reinterpret_cast<const short *>(L.W);
                // (the keys of one round, by reference: two plain rounds of a trip meet the running minima in one v_min3_u32 per slot)
                auto scan_round2 = [&](auto with_w, int base, int rd, int w, int rt, uint32_t &key1, uint32_t &key2) {
                    const uint32_t st1 = lcg24(rng);
                    uint32_t st2;
                    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(st2) : "v"(st1), "s"(jmp_a), "v"(jc));
                    const int inc = wfld(w, kWIncR);
                    if constexpr (kSmall) {
                        // (inc + incL * lead1 | inc + incL * lead2) + RT's word, times lam, plus (K01 | K02): three packed instructions
                        uint32_t d = pk_mad_ss(pk_add(pk_mad_lo((uint32_t)wfld(w, kWIncL), leadp, (uint32_t)inc), (uint32_t)rt), (uint32_t)lam, K0p);
                        if (decltype(with_w)::value) {
                            const uint32_t x = (uint32_t)(base + lane);
                            const uint32_t xw = x | ((uint32_t)XR[x] << 16);
                            // role_w2 of both slots, each weight already scaled and in its slot's half: a mask per (slot, role) AND-ed with
                            // the wave-uniform weight (a select would copy each of the four scalars into a VGPR first).  A partition's
                            // current replicas are distinct brokers (kao_model.cpp refuses anything else): at most one mask per slot is set.
                            auto mask_of = [](bool b) { uint32_t m = b ? ~0u : 0u; asm("" : "+v"(m)); return m; };
                            const bool l1 = c1.w[0] == xw, l2 = c2.w[0] == xw;
                            bool f1 = false, f2 = false;
#pragma unroll
                            for (int i2 = 1; i2 < NS; ++i2) { f1 |= c1.w[i2] == xw; f2 |= c2.w[i2] == xw; }
                            auto and_or = [](uint32_t m, uint32_t w, uint32_t acc) { uint32_t r; asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "s"(w), "v"(acc)); return r; };
                            uint32_t ws = mask_of(l1) & (uint32_t)wl1h;
                            ws = and_or(mask_of(f1), (uint32_t)wf1h, ws);
                            ws = and_or(mask_of(l2), (uint32_t)wl2s, ws);
                            ws = and_or(mask_of(f2), (uint32_t)wf2s, ws);
                            d = pk_sub(d, ws);
                        }
                        // no candidate: slot 1's half all ones from the sign-extended word, slot 2's from bit 14
                        key1 = ((d | (uint32_t)w) & 0xFFFF0000u) | (st1 & 0xFF00u) | (uint32_t)rd;
                        key2 = ((d | (uint32_t)wflag(w, 14)) << 16) | (st2 & 0xFF00u) | (uint32_t)rd;
                        return;
                    }
                    int d1 = __mul24(lam, inc + wfldw(w, kWIncL, lw1) + wfldw(rt, 0, 16u)) + K01;
                    int d2 = __mul24(lam, inc + wfldw(w, kWIncL, lw2) + (rt >> 16)) + K02;
                    if (decltype(with_w)::value) {
                        const uint32_t x = (uint32_t)(base + lane);
                        const uint32_t xw = x | ((uint32_t)XR[x] << 16);
                        d1 -= __mul24(S, role_w2<NS>(c1, xw, wl1, wf1));
                        d2 -= __mul24(S, role_w2<NS>(c2, xw, wl2, wf2));
                    }
                    d1 = min(max(d1, 0), 2 * kDBias - 2);
                    d2 = min(max(d2, 0), 2 * kDBias - 2) | wflag(w, 14);   // slot 2's no-candidate bit: all ones, a cost field of 0xFFFF below
                    key1 = ((uint32_t)d1 << 16) | (st1 & 0xFF00u) | (uint32_t)rd | ((uint32_t)w & 0xFFFF0000u);
                    key2 = ((uint32_t)d2 << 16) | (st2 & 0xFF00u) | (uint32_t)rd;
                };
                const int n_rd = (T.Bx + 63) >> 6;
                int rd = 0, base = 0;
                while (rd < n_rd) {
                    int nxt = n_rd;   // the next round with a displaced current replica of either slot
#pragma unroll
                    for (int i2 = 0; i2 < 2 * NW; ++i2)
                        if (mr[i2] >= rd) nxt = min(nxt, mr[i2]);
                    uint32_t k1a, k2a, k1b, k2b;
                    for (; rd + 1 < nxt; rd += 2, base += 128) {   // two rounds share the address arithmetic, as in the one-slot scan below
                        const int wa = Ws[base + lane], wb = Ws[base + 64 + lane];
                        const uint32_t ra = XR[base + lane], rb = XR[base + 64 + lane];
                        const int rta = L.RT[ra], rtb = L.RT[rb];
                        scan_round2(std::false_type{}, base, rd, wa, rta, k1a, k2a);
                        scan_round2(std::false_type{}, base + 64, rd + 1, wb, rtb, k1b, k2b);
                        best1 = min(best1, min(k1a, k1b));
                        best2 = min(best2, min(k2a, k2b));
                    }
                    if (rd < nxt) { const int wa = Ws[base + lane]; scan_round2(std::false_type{}, base, rd, wa, L.RT[XR[base + lane]], k1a, k2a); best1 = min(best1, k1a); best2 = min(best2, k2a); ++rd; base += 64; }
                    if (rd < n_rd) { const int wa = Ws[base + lane]; scan_round2(std::true_type{}, base, rd, wa, L.RT[XR[base + lane]], k1a, k2a); best1 = min(best1, k1a); best2 = min(best2, k2a); ++rd; base += 64; }
                }
                asm("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(rng) : "s"(jmp_a), "v"(jc));   // state after both slots' 2 n_rd draws
                if (holds) L.W[ai & 0xFFFFu] = (uint16_t)w_keep;
                // one reduction picks slot and lane: key (24 bits: (cost + bias) << 8 | tie) << 7 | slot << 6 | lane.  Its minimum is the
                // lowest key; ties go to slot 1, then to the lowest lane -- the rule of two minima, a compare and a ballot.
                const uint32_t kw = wave_umin(min(((best1 >> 1) & ~127u) | (uint32_t)lane, ((best2 >> 1) & ~127u) | 64u | (uint32_t)lane));
                const bool two = (kw & 64u) != 0u;   // wave-uniform
                const uint32_t kmin = kw >> 7;
                const int win = (int)(kw & 63u);
                const int p = two ? ps[1] : ps[0], k = two ? ks[1] : ks[0];
                const uint32_t uw = two ? us[1] : us[0];
                if ((int)(kmin >> 8) - kDBias <= 0) {   // will be accepted: the winner's move, wave-uniform -- p, k, uw as scalars
                    const bool lead = k == 0;
                    const uint32_t bw_ = (uint32_t)__builtin_amdgcn_readlane((int)(two ? best2 : best1), win);
                    const uint32_t xs = ((bw_ & 255u) << 6) + (uint32_t)win;
                    const uint32_t rs = XR[xs];
                    const uint32_t ws = L.W[xs];
                    const int rts = L.RT[rs];
                    const uint32_t vw = xs | (rs << 16);
                    const int dV = wfld(ws, kWIncR) + wfldw(ws, kWIncL, lead ? 2u : 0u) + (two ? dvos[1] : dvos[0]) + ((two != kSmall) ? (rts >> 16) : wfldw(rts, 0, 16u));
                    int mx1 = -1, mx2 = -1;   // (each slot's own maximum, then a select: `two ? mr[NW + i2] : mr[i2]` became a dynamically indexed scratch array)
#pragma unroll
                    for (int i2 = 0; i2 < NW; ++i2) { mx1 = max(mx1, mr[i2]); mx2 = max(mx2, mr[NW + i2]); }
                    const bool has_missing = (two ? mx2 : mx1) >= 0;
                    const int dObj = -(two ? gs[1] : gs[0]) + (has_missing ? (two ? role_w2<NS>(c2, vw, wl2, wf2) : role_w2<NS>(c1, vw, wl1, wf1)) : 0);
                    finish(kReplace, std::true_type{}, kmin, win, p, k, 0, 0, uw, vw, dV, dObj);
                }
            } else {
            // the slot (p,k) of tournament lane wA, wave-uniform: what taking its replica out is worth, and its partition's words
            auto slot_of = [&](int wA, int &p, int &k, uint32_t &uw, int &g_old, int &dV_old, int &dV_rack_old, Part<NW> &a, Part<NW> &c) {
                p = __builtin_amdgcn_readlane(pl_, wA);
                k = __builtin_amdgcn_readlane(kl_, wA);
                uw = (uint32_t)__builtin_amdgcn_readlane((int)oldw_l, wA);
                g_old = __builtin_amdgcn_readlane(g_old_l, wA);
                dV_old = __builtin_amdgcn_readlane(dvo_l, wA);
                dV_rack_old = __builtin_amdgcn_readlane(dvr_l, wA);
                if constexpr (kGlobalA) {
#pragma unroll
                    for (int i2 = 0; i2 < NW; ++i2) { a.w[i2] = (uint32_t)__builtin_amdgcn_readlane((int)a_l.w[i2], wA); c.w[i2] = (uint32_t)__builtin_amdgcn_readlane((int)c_l.w[i2], wA); }
                } else {
                    a = L.A[p];   // same address in every lane: LDS broadcast
                    c = CUR[p];
                }
            };
            if (type == 0) {
            // the move of the first slot is final when it is the only one; a second slot's replaces it when its wave minimum is lower
            uint32_t b_kmin = kKeyNull, b_uw = 0, b_vw = 0;
            int b_win = 0, b_p = 0, b_k = 0, b_dV = 0, b_dObj = 0;
#pragma nounroll
            for (int si = 0; si < (wA2 >= 0 ? 2 : 1); ++si) {
                int p, k, g_old, dV_old, dV_rack_old;
                uint32_t uw;
                Part<NW> a, c;
                slot_of(si == 0 ? wA1 : wA2, p, k, uw, g_old, dV_old, dV_rack_old, a, c);
                const bool lead = k == 0;  // wave-uniform
                const uint32_t ro = uw >> 16;
                uint32_t vw = 0;   // the winner's move, recomputed in every lane: wave-uniform like p, k, uw
                int dV = 0, dObj = 0;
                // ---- phase B (REPLACE): every target broker for slot (p,k), 64 per round -- the band-state scan.  A candidate
                //      costs one W read (band deltas + where its rack's entry of RT lives), one RT read, two bit-field
                //      extracts, the cost and the key; the per-lane running minimum is a plain v_min_u32 because the key carries
                //      the round number below the tie bits; only the winner's details are recomputed afterwards.  Same
                //      candidates, same keys, same winner as the scalar restatement (oracle/kao_port.c).
                {   // rack-dependent part of the delta, racks strided over the lanes
                    const int dP_rack_old = kPriced ? p_out(L.K[ro], T.rack_lo, T.rack_hi, PG[ro]) : 0;
                    for (int r = lane; r < T.R; r += 64) {
                        int v = ((uint32_t)r != ro) ? dV_rack_old + dinc(L.K[r], T.rack_lo, T.rack_hi) + c7_delta(T.c7_inc, cnt4x2<NS>(a, (uint32_t)r)) : 0;
                        if (kPriced)  // rack part of the price delta rides in the upper 24 bits (the violation delta is within -8..8)
                            v = (v & 0xFF) | ((((uint32_t)r != ro) ? dP_rack_old + p_in(L.K[r], T.rack_lo, T.rack_hi, PG[r]) : 0) * 256);
                        L.RT[r] = v;
                    }
                }
                const int wl = lead ? T.w00 : T.w01, wf = lead ? T.w10 : T.w11;
                // lane i < NW looks after slot i of the partition: (1) the broker it holds is no candidate (row C5) -- for the
                // duration of the scan its W entry points at the reserved RT entry; (2) current replica i, when displaced (in c,
                // not in a), is the only broker with a non-zero objective weight here: the round it falls into is scored with weights
                const int li = lane & (NW - 1);
                const uint32_t ai = sel_slot<NS>(a, li), ci = sel_slot<NS>(c, li);
                // (a team shares W: nothing may be marked there -- the rounds that hold a broker of the partition take the slow
                //  path below, like the rounds with a displaced current replica, and drop it by comparison)
                const bool holds = (lane < NS) & (ai != kNoneW);
                uint32_t w_keep = 0;
                if (!kTeam && holds) {
                    w_keep = L.W[ai & 0xFFFFu];
                    L.W[ai & 0xFFFFu] = (uint16_t)(w_keep | kWNoCand);
                }
                int ar[NS];
                {
                    const int ar_l = (kTeam && holds) ? (int)((ai & 0xFFFFu) >> 6) : -1;
#pragma unroll
                    for (int i2 = 0; i2 < NS; ++i2) ar[i2] = __builtin_amdgcn_readlane(ar_l, i2);
                }
                const bool hm_l = (lane < NS) & (ci != kNoneW) & !in4<NS>(a, ci);
                const int mr_l = hm_l ? (int)((ci & 0xFFFFu) >> 6) : -1;
                int mr[NS];
#pragma unroll
                for (int i2 = 0; i2 < NS; ++i2) mr[i2] = __builtin_amdgcn_readlane(mr_l, i2);
                bool has_missing = false;
#pragma unroll
                for (int i2 = 0; i2 < NS; ++i2) has_missing |= mr[i2] >= 0;
                // cost + bias of a candidate = lam * (its own delta + dV_old) + S * g_old (+ prices) (- S * weight of a displaced
                // current replica): everything that does not depend on the candidate is one wave-uniform constant
                int K0 = __mul24(S, g_old) + kDBias + __mul24(lam, dV_old);
                if (kPriced) {
                    const uint32_t pro = PR[uw & 0xFFFFu];
                    const uint32_t wo = L.W[uw & 0xFFFFu];
                    K0 -= wflag(wo, kWPoutR) & price_rep(pro);
                    if (lead) K0 -= wflag(wo, kWPoutL) & price_lead(pro);
                }
                const uint32_t lw = lead ? 2u : 0u, lf = lead ? 1u : 0u;   // widths of the leader fields / flags: zero for follower slots
                uint32_t bestA = kKeyNull;   // (cost + bias) << 16 | tie << 8 | round within the chunk of 256 rounds
                int chunkA = 0;
                // one round: 64 candidates x = base + lane, `rd` = round within the chunk of 256; `with_w` (compile time): the
                // round holds a displaced current replica of the partition and is scored with objective weights
                // (a round's loads apart from its arithmetic, as in the fused scan: `w` = W of the lane's index, sign-extended so that
                //  bit 15 fills the upper half, `rt` = RT of its rack; a trip of two rounds issues each kind together)
                const short *Ws = reinterpret_cast<const short *>(L.W);
                auto scan_round_on = [&](auto with_w, int base, int rd, int w, int rt) -> uint32_t {
                    const uint32_t st = lcg24(rng);   // tie bits = bits 8..15 of the draw, as make_key_tie(lcg24 >> 8)
                    int dsc;
                    if (kPriced) {   // RT entry: violation delta in the low byte, rack price above it
                        const uint32_t prx = PR[base + lane];
                        const int dVx = wfld(w, kWIncR) + wfldw(w, kWIncL, lw) + (int)(signed char)(rt & 0xFF);
                        dsc = __mul24(lam, dVx) + K0 + (rt >> 8) + (wflag(w, kWPinR) & price_rep(prx)) + (wflagw(w, kWPinL, lf) & price_lead(prx));
                        if (hbw) dsc -= __mul24(S, bw_of(BW[base + lane], lead));
                    } else {
                        const int dVx = wfld(w, kWIncR) + wfldw(w, kWIncL, lw) + rt;
                        dsc = __mul24(lam, dVx) + K0;
                    }
                    uint32_t member = 0;
                    if (decltype(with_w)::value) {
                        const uint32_t x = (uint32_t)(base + lane);
                        const uint32_t xw = x | ((uint32_t)XR[x] << 16);
                        dsc -= __mul24(S, role_w2<NS>(c, xw, wl, wf));
                        if (kTeam && in4<NS>(a, xw)) member = 0xFFFF0000u;   // row C5: already in the partition
                    }
                    dsc = min(max(dsc, 0), 2 * kDBias - 2);
                    // a "no candidate" index gets a cost field of 0xFFFF: above every real cost (<= 2 * kDBias - 2) and never accepted
                    return ((uint32_t)dsc << 16) | (st & 0xFF00u) | (uint32_t)rd | ((uint32_t)w & 0xFFFF0000u) | member;
                };
                auto scan_round = [&](auto with_w, int base, int rd) -> uint32_t {
                    const int w = Ws[base + lane];
                    return scan_round_on(with_w, base, rd, w, L.RT[XR[base + lane]]);
                };
                // two plain rounds of one trip, their minimum
                auto scan_pair = [&](int base, int rd) -> uint32_t {
                    const int wa = Ws[base + lane], wb = Ws[base + 64 + lane];
                    const uint32_t ra = XR[base + lane], rb = XR[base + 64 + lane];
                    const int rta = L.RT[ra], rtb = L.RT[rb];
                    const uint32_t k0 = scan_round_on(std::false_type{}, base, rd, wa, rta);
                    const uint32_t k1 = scan_round_on(std::false_type{}, base + 64, rd + 1, wb, rtb);
                    return min(k0, k1);
                };
                auto is_weighted = [&](int rdg) {   // wave-uniform
                    bool wgt = false;
#pragma unroll
                    for (int i2 = 0; i2 < NS; ++i2) wgt |= (mr[i2] == rdg) | (kTeam && ar[i2] == rdg);
                    return wgt;
                };
                for (int cb = 0; cb < T.Bx; cb += 16384) {
                    uint32_t bestc = kKeyNull;
                    const int cend = min(T.Bx, cb + 16384);
                    int rd = 0, base = cb;
                    if (kWide) {   // two rounds per trip: straight-line code, the LDS round trips of one round hide behind the other's
                        for (; base + 64 < cend; base += 128, rd += 2) {
                            const int rdg = (cb >> 6) + rd;
                            if (is_weighted(rdg) || is_weighted(rdg + 1)) {   // rare: at most NW rounds of a scan carry weights
                                bestc = min(bestc, is_weighted(rdg) ? scan_round(std::true_type{}, base, rd) : scan_round(std::false_type{}, base, rd));
                                bestc = min(bestc, is_weighted(rdg + 1) ? scan_round(std::true_type{}, base + 64, rd + 1) : scan_round(std::false_type{}, base + 64, rd + 1));
                            } else bestc = min(bestc, scan_pair(base, rd));
                        }
                    }
                    if (kWide || kTeam) {
                        for (; base < cend; base += 64, ++rd)
                            bestc = min(bestc, is_weighted((cb >> 6) + rd) ? scan_round(std::true_type{}, base, rd) : scan_round(std::false_type{}, base, rd));
                    } else {
                        // Round 5: the rounds between two weighted ones run in a loop of their own.  Asking every round
                        // "is it one of the NW weighted ones" was 11 of its 22 scalar instructions -- and the two-way
                        // body cost two register copies of the generator state and an address add per round on top of
                        // the 12 vector instructions a candidate round needs.  Same rounds, same order, same draws.
                        const int n_rd = (cend - cb + 63) >> 6, rd0 = cb >> 6;
                        while (rd < n_rd) {
                            int nxt = n_rd;   // the next weighted round of this chunk at or after rd
#pragma unroll
                            for (int i2 = 0; i2 < NS; ++i2) {
                                const int m = mr[i2] - rd0;
                                if (m >= rd) nxt = min(nxt, m);
                            }
                            for (; rd + 1 < nxt; rd += 2, base += 128) bestc = min(bestc, scan_pair(base, rd));   // two rounds share the address arithmetic and one v_min3_u32
                            if (rd < nxt) { bestc = min(bestc, scan_round(std::false_type{}, base, rd)); ++rd; base += 64; }
                            if (rd < n_rd) { bestc = min(bestc, scan_round(std::true_type{}, base, rd)); ++rd; base += 64; }
                        }
                    }
                    if ((bestc >> 8) < (bestA >> 8)) { bestA = bestc; chunkA = cb; }   // strict: ties stay with the earlier round
                }
                if (!kTeam && holds) L.W[ai & 0xFFFFu] = (uint16_t)w_keep;
                const uint32_t key = bestA >> 8;   // (cost + bias) << 8 | tie: the key format of every other move type
                const uint32_t kmin = wave_umin(key);
                const unsigned long long bal = __ballot(key == kmin);
                const int win = __ffsll((long long)bal) - 1;  // ties inside the wave go to the lowest lane
                if ((int)(kmin >> 8) - kDBias <= 0) {   // will be accepted: the winner's move, wave-uniform
                    const uint32_t bw_ = (uint32_t)__builtin_amdgcn_readlane((int)bestA, win);
                    const uint32_t xs = (uint32_t)__builtin_amdgcn_readlane(chunkA, win) + ((bw_ & 255u) << 6) + (uint32_t)win;
                    const uint32_t rs = XR[xs];
                    const uint32_t ws = L.W[xs];
                    const int rts = L.RT[rs];
                    vw = xs | (rs << 16);
                    dV = wfld(ws, kWIncR) + wfldw(ws, kWIncL, lw) + dV_old + (kPriced ? (int)(signed char)(rts & 0xFF) : rts);
                    dObj = -g_old + (has_missing ? role_w2<NS>(c, vw, wl, wf) : 0) + (hbw ? bw_of(BW[xs], lead) : 0);
                }
                if (si == 0 || kmin < b_kmin) { b_kmin = kmin; b_win = win; b_p = p; b_k = k; b_uw = uw; b_vw = vw; b_dV = dV; b_dObj = dObj; }
            }   // (the two scan slots)
            finish(kReplace, std::true_type{}, b_kmin, b_win, b_p, b_k, 0, 0, b_uw, b_vw, b_dV, b_dObj);
            } else {
                // ---- phase B (EXCHANGE): every partner slot (q,j) for slot (p,k), 64 partitions per round ----
                int p, k, g_old, dV_old, dV_rack_old;
                uint32_t uw;
                Part<NW> a, c;
                slot_of(wA1, p, k, uw, g_old, dV_old, dV_rack_old, a, c);
                const bool lead = k == 0;  // wave-uniform
                const uint32_t ro = uw >> 16;
                uint32_t key = kKeyNull, vw = 0;   // this lane's best partner slot
                int dV = 0, dObj = 0, q = 0, j = 0;
                const int nrp = lead ? 0 : 1;
                const int cnt_a_ru2 = cnt4x2<NS>(a, ro);   // (counts in twos: c7_delta)
                const uint32_t wu = L.W[uw & 0xFFFFu];
                const int pl_u = kPriced ? price_lead(PR[uw & 0xFFFFu]) : 0;
                const int bwl_u = hbw ? (int)(BW[uw & 0xFFFFu] >> 16) : 0;
                // every lane draws; lane 0's value places the window when the topic has more than 512 partitions
                // (topics in global memory: drawn -- at the same place of the stream -- and its first partner words loaded by tournament_global)
                if (!kGlobalA) {
                    const int q_draw = (int)rnd24_wide(rng, (uint32_t)T.P);
                    q0 = x_windowed ? __builtin_amdgcn_readfirstlane(q_draw) : 0;
                }
                const int x_rounds = x_windowed ? 8 : x_rounds_full;
                auto x_round = [&](int rd, const Part<NW> &b, const Part<NW> &cb) {
                    const uint32_t tie0 = lcg24(rng) >> 8;
                    int qq; bool okq;
                    x_partner(rd, qq, okq);
                    okq = okq & (qq != p);
                    const bool u_in_b = in4<NS>(b, uw);
                    // independent of the partner slot j: what u would be worth in q, and q's replicas in u's rack
                    const int u_in_q_lead = role_w2<NS>(cb, uw, T.w00, T.w10), u_in_q_fol = role_w2<NS>(cb, uw, T.w01, T.w11);
                    // what leaving rack ro costs (u leaves a, a replica in ro joins b): the same for every partner slot in another rack
                    const int dv_ro = c7_delta(T.c7_dec, cnt_a_ru2) + c7_delta(T.c7_inc, cnt4x2<NS>(b, ro));
                    // replicas of q in the rack of each partner slot, in twos.  Three slots (RFT = 3): the three pairwise rack equalities give all
                    // three counts (an empty word's rack, 0xFFFF, equals only another empty word's, as in cnt4); otherwise counted per slot
                    int cnt_b_rv[3] = {0, 0, 0};
                    if constexpr (RFT == 3) {
                        const int e01 = (int)((b.w[0] >> 16) == (b.w[1] >> 16)), e02 = (int)((b.w[0] >> 16) == (b.w[2] >> 16)), e12 = (int)((b.w[1] >> 16) == (b.w[2] >> 16));
                        cnt_b_rv[0] = (1 + e01 + e02) << 1; cnt_b_rv[1] = (1 + e01 + e12) << 1; cnt_b_rv[2] = (1 + e02 + e12) << 1;
                    }
#pragma unroll
                    for (int jj = 0; jj < NS; ++jj) {
                        if (!RFT && jj >= T.RF) break;
                        const uint32_t v = b.w[jj];
                        const bool ok = okq & (v != uw) & !in4<NS>(a, v) & !u_in_b;
                        const int nrq = jj != 0;
                        int dObjx = role_w<NS>(T, c, v, nrp) + (jj == 0 ? u_in_q_lead : u_in_q_fol) - g_old - role_w<NS>(T, cb, v, nrq);
                        int dVx = 0, dPx = 0;
                        if (lead != (jj == 0)) {  // wave-uniform: exactly one of the two slots is a leader slot
                            const uint32_t wv = L.W[v & 0xFFFFu];
                            dVx += lead ? (wfld(wu, kWDecL) + wfld(wv, kWIncL)) : (wfld(wv, kWDecL) + wfld(wu, kWIncL));
                            if (kPriced) {  // the leader moves u -> v or v -> u
                                if (hbw) { const int dbl = (int)(BW[v & 0xFFFFu] >> 16) - bwl_u; dObjx += lead ? dbl : -dbl; }
                                const int plv = price_lead(PR[v & 0xFFFFu]);
                                dPx = lead ? ((wflag(wv, kWPinL) & plv) - (wflag(wu, kWPoutL) & pl_u))
                                           : ((wflag(wu, kWPinL) & pl_u) - (wflag(wv, kWPoutL) & plv));
                            }
                        }
                        const uint32_t rv = v >> 16;
                        if (rv != ro)
                            dVx += dv_ro + c7_delta(T.c7_inc, cnt4x2<NS>(a, rv)) + c7_delta(T.c7_dec, RFT == 3 ? cnt_b_rv[jj < 3 ? jj : 0] : cnt4x2<NS>(b, rv));
                        uint32_t keyx;
                        if constexpr (kSmall) keyx = ok ? key_small(mad24s(lam, dVx, mad24s(-S, dObjx, kDBias)), (tie0 + (uint32_t)jj * 0x55u) & 0xFFu) : kKeyNull;
                        else if (kPriced) keyx = ok ? make_key_tie_p(lam, S, dVx, dObjx, dPx, tie0 + (uint32_t)jj * 0x55u) : kKeyNull;
                        else keyx = ok ? make_key_tie(lam, S, dVx, dObjx, tie0 + (uint32_t)jj * 0x55u) : kKeyNull;
                        if (keyx < key) { key = keyx; vw = v; q = qq; j = jj; dV = dVx; dObj = dObjx; }
                    }
                };
                if constexpr (kGlobalA) {
#pragma unroll
                    for (int r2 = 0; r2 < XB; ++r2)
                        if (r2 < x_rounds) x_round(r2, xb[r2], xcb[r2]);
                    for (int rb = XB; rb < x_rounds; rb += XB) {   // (8 words per partition: the second half of the rounds)
                        Part<NW> yb[XB], ycb[XB];
#pragma unroll
                        for (int r2 = 0; r2 < XB; ++r2) { int qq; bool okq; const int qc = x_partner(rb + r2, qq, okq); yb[r2] = L.A[qc]; ycb[r2] = CUR[qc]; }
#pragma unroll
                        for (int r2 = 0; r2 < XB; ++r2)
                            if (rb + r2 < x_rounds) x_round(rb + r2, yb[r2], ycb[r2]);
                    }
                } else {
                    for (int rd = 0; rd < x_rounds; ++rd) {
                        int qq; bool okq;
                        const int qc = x_partner(rd, qq, okq);
                        const Part<NW> b = L.A[qc];
                        const Part<NW> cb = CUR[qc];
                        x_round(rd, b, cb);
                    }
                }
                const uint32_t kmin = wave_umin(key);
                const unsigned long long bal = __ballot(key == kmin);
                const int win = __ffsll((long long)bal) - 1;  // ties inside the wave go to the lowest lane
                finish(kExchange, std::false_type{}, kmin, win, p, k, q, j, uw, vw, dV, dObj);
            }
            }   // (one slot at a time)
        }
        // (V, obj: as the iteration's move, if any, left them.  Both are scalars, and so is best_obj: snapshot() loops a wave-uniform
        //  number of times, so this branch stays a scalar one and what is set behind it a scalar)
        if (V == 0 && obj > best_obj) { best_obj = obj; snapshot(T, L, ext, best, tid, nthr); }
    }

    // ---- end of launch: verify the incremental bookkeeping against a from-scratch recount ----
    if (kTeam) __syncthreads();
    recount(T, L, tid, nthr, krt);
    if (kTeam) __syncthreads();
    int V2, obj2;
    T = topic_regs<RFT>(TD);   // (the band ends: not kept across the loop)
    full_cost<NW, kTeam>(T, L, CUR, RSZ, tid, nthr, V2, obj2, hbw ? BW : nullptr, TS, wave, n_waves);
    // (the chunked instantiation reads the arguments it needs behind the loop there: late_kernarg)
    if ((V2 != V || obj2 != obj) && tid == 0) atomicAdd(kChunked ? late_kernarg<int32_t *>(offsetof(SearchPools, drift)) : pl.drift, 1);
    if (!kGlobalA)
        for (int p = lane; p < T.P; p += 64) store_packed<NW>(state_packed, p, L.A[p]);
    if (tid == 0) {
        int32_t *info = (kChunked ? late_kernarg<int32_t *>(offsetof(SearchPools, restart_info)) : pl.restart_info) + g * 4;
        info[0] = best_obj;
        info[1] = V2;
        info[2] = obj2;
        info[3] = accepted;
    }
    if constexpr (kCanChunk) {   // chunked launch: the generator words for the chunk behind this one (the last chunk's are never read)
        uint32_t *words = late_kernarg<uint32_t *>(offsetof(SearchPools, chunk_rng)) + (size_t)g * 64 + lane;
        const uint32_t ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)*words);
        *words = rng;
        chunk_pass(ticket);
    }
}

// ---- a launch as ticketed chunks ----
// chunk_take: the workgroup takes the next ticket and looks its piece up in the schedule.  The schedule lists the chunks of one entry in
// increasing ticket order, so the chunk before this one was taken by a workgroup that is already running (or has finished): waiting for
// its record cannot deadlock, and a first chunk never waits.  The wait is bounded all the same: after kChunkPolls polls the workgroup
// counts itself in the error word behind `drift`, marks the entry as given up and runs nothing; the entry's later chunks see the mark
// and do the same at once, so the kernel always ends and the session reports the error at its next synchronising call.
// Returns false when the workgroup has nothing to run.  `smem`: two words at the start of the carve, free before the body stages.
constexpr uint32_t kChunkPolls = 1u << 22;   // x (s_sleep 16 + one load that misses the caches) = several seconds: hundreds of launches
__device__ __forceinline__ bool chunk_take(unsigned char *smem, const SearchPools &pl, const SearchParams &prm, SearchPiece &pc, uint32_t &ticket) {
    uint32_t *bc = reinterpret_cast<uint32_t *>(smem);
    if (threadIdx.x == 0) {
        const uint32_t t = atomicAdd(pl.chunk_ticket, 1u);
        if (t + 1u == gridDim.x) __hip_atomic_store(pl.chunk_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every ticket is out: ready for the next launch
        const int4 sc = pl.chunk_sched[t];
        const uint32_t c = (uint32_t)sc.y & 0xFFu, nc = (uint32_t)sc.y >> 8;
        uint32_t ok = 1u;
        if (c > 0u) {
            uint32_t *word = pl.chunk_progress + sc.x;
            const uint32_t want = prm.serial * 256u + c, gone = prm.serial * 256u + kChunkPoison;
            for (uint32_t n = 0;; ++n) {
                const uint32_t v = __hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                if (v == want) break;
                if (v == gone || n >= kChunkPolls) { ok = 0u; break; }
                __builtin_amdgcn_s_sleep(16);
            }
            if (!ok) {
                atomicAdd(pl.drift + 1, 1);
                if (c + 1u < nc) __hip_atomic_store(word, gone, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        bc[0] = t; bc[1] = ok;
    }
    __syncthreads();
    ticket = (uint32_t)__builtin_amdgcn_readfirstlane((int)bc[0]);
    const bool ok = __builtin_amdgcn_readfirstlane((int)bc[1]) != 0;
    __syncthreads();   // (the two words are the start of the carve: the body stages over them)
    // every wavefront: no load of the predecessor's record (packed state, restart_info, generator words) before this point
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const int4 sc = sched_record(pl.chunk_sched, ticket);
    const bool later = ((uint32_t)sc.y & 0xFFu) != 0u;
    pc = SearchPiece{(uint32_t)sc.x, later ? 0 : prm.init, later ? 0 : prm.elite, (uint32_t)sc.z, (uint32_t)sc.w, later, ticket};
    return ok;
}
// chunk_pass: at the end of the body, every wavefront of the workgroup (one without a restart too, from where the body returns early
// for it: it must not miss the barrier).  Every wavefront's stores are released at agent scope -- the chunks of one entry land on different compute
// units and XCDs --, the workgroup meets, and thread 0 publishes the entry's count of finished chunks.
__device__ __forceinline__ void chunk_pass(uint32_t ticket) {
    const int4 sc = sched_record(late_kernarg<const int4 *>(offsetof(SearchPools, chunk_sched)), ticket);
    const uint32_t c = (uint32_t)sc.y & 0xFFu, nc = (uint32_t)sc.y >> 8;
    if (c + 1u >= nc) return;   // the last chunk: nobody waits for it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_store(late_kernarg<uint32_t *>(offsetof(SearchPools, chunk_progress)) + sc.x,
                           late_kernarg<uint32_t>(kArgPrm + offsetof(SearchParams, serial)) * 256u + c + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

#ifndef KAO_WPE_SMALL
#define KAO_WPE_SMALL 6
#endif
#ifndef KAO_WPE_WIDE
#define KAO_WPE_WIDE 6
#endif
template <bool kGlobalA, bool kPriced, int NW, bool kWide> constexpr int search_min_waves() { return kGlobalA ? 1 : (kWide ? KAO_WPE_WIDE : KAO_WPE_SMALL); }
template <bool kGlobalA, bool kPriced, int NW, bool kWide, int RFT = 0, bool kSmall = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(search_min_waves<kGlobalA, kPriced, NW, kWide>(), 8))) void k_search(SearchPools pl, SearchParams prm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    search_body<kGlobalA, kPriced, NW, kWide, false, false, RFT, kSmall>(smem, pl, prm, whole_launch(prm));
}
// the same for a chunked launch (LDS-resident topics): one workgroup per ticket.  Its arguments are (SearchPools, SearchParams), in that
// order and nothing else: late_kernarg reads them by offset.
template <bool kPriced, int NW, bool kWide, int RFT = 0, bool kSmall = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(search_min_waves<false, kPriced, NW, kWide>(), 8))) void k_search_chunked(SearchPools pl, SearchParams prm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    SearchPiece pc;
    uint32_t ticket;
    if (!chunk_take(smem, pl, prm, pc, ticket)) return;   // (wave-uniform: a word broadcast through LDS)
    search_body<false, kPriced, NW, kWide, false, false, RFT, kSmall, true>(smem, pl, prm, pc);
}
static_assert(std::is_same_v<decltype(&k_search_chunked<false, 4, false, 3, true>), void (*)(SearchPools, SearchParams)> &&
              std::is_same_v<decltype(&k_search_chunked<true, 8, true>), void (*)(SearchPools, SearchParams)>,
              "late_kernarg reads k_search_chunked's arguments by offset: (SearchPools, SearchParams) by value, in that order, nothing else");
// working assignment in LDS, current assignment from global memory / L2 (kCurG; ~4,900 .. 9,800 partitions: always wide)
template <bool kPriced, int NW>
__global__ __launch_bounds__(256) void k_search_curg(SearchPools pl, SearchParams prm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    search_body<false, kPriced, NW, true, false, true>(smem, pl, prm, whole_launch(prm));
}
// a team of up to 8 wavefronts per restart (topics in global memory; see search_body)
template <bool kPriced, int NW>
__global__ __launch_bounds__(NW == 8 ? 256 : 512) void k_team(SearchPools pl, SearchParams prm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    search_body<true, kPriced, NW, true, true>(smem, pl, prm, whole_launch(prm));
}

// ------------------------------------------------------------------------------------------------
// K-init (round 6): the hole filling of an initialising launch, one WORKGROUP per restart -- topics in global memory only
// ------------------------------------------------------------------------------------------------
// search_body fills the holes with ONE wavefront per restart: every hole scans all Bx brokers, 64 per round, and the holes are a chain
// (each insertion moves the counters the next one reads) -- 15,000 holes x 16 rounds = 70 ms for config 5 as one topic, on a quarter
// of the chip's SIMDs at best.  Here the rounds of a hole are dealt to the W wavefronts of the workgroup (round j to wavefront j mod W);
// every wavefront reduces its rounds to one record (key, lane, round, word), the records meet in LDS behind ONE workgroup barrier per hole
// and every wavefront takes the same minimum in the order of the single-wavefront scan: lowest key, then lowest lane, then -- inside a
// lane -- the earliest round.  Same holes, same order, same winners -- the replays (oracle/kao_port.c::ls_init) hold bit for bit; k_search / k_team
// then run with prm.init = 2 (state seeded and filled, everything else as in an initialising launch).
constexpr int kInitWaves = 16;
// the carve at the top of k_init ("LDS:"), summed (pinned below)
constexpr size_t init_lds_total(size_t maxBx, int maxR, bool priced, bool bw) {
    const size_t bx64 = (maxBx + 63) & ~(size_t)63, krt = (size_t)search_rack_tab(maxR);
    return krt * 4 + bx64 + (priced ? (bw ? 2 : 1) * bx64 * 4 + krt * 4 : 0) + bx64 * 4 + krt * 4 + (size_t)kInitWaves * krt * 4 + 3 * 8;
}
size_t init_lds_bytes(int maxBx, int maxR, bool priced, bool bw) { return init_lds_total((size_t)maxBx, maxR, priced, bw); }
static_assert(init_lds_total(500, 255, false, false) == 21016 && init_lds_total(500, 255, true, true) == 26136, "init_lds_total no longer sums the LDS carve of k_init");   // 255 racks
template <bool kPriced, int NW>
__global__ __launch_bounds__(64 * kInitWaves) void k_init(SearchPools pl, SearchParams prm, int per_block) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int2 bm = pl.block_map[blockIdx.x / (unsigned)per_block];
    const TopicDev *TD = pl.topics + bm.x;
    const int rho = bm.y + (int)(blockIdx.x % (unsigned)per_block);
    if (rho >= TD->n_restarts) return;   // (the whole workgroup)

    const TopicRegs T = topic_regs(TD);

    // LDS: [RSZ int[krt]] [XR u8[bx64]] ([PR u32[bx64]] [PG int[krt]] ([BW u32[bx64]])) [C u32[bx64]] [K int[krt]] [KW int[W][krt]] [BEST u64[3]]
    const int bx64 = (prm.maxBx + 63) & ~63, krt = search_rack_tab(prm.maxR);
    const bool hbw = kPriced && prm.bw != 0;
    const uint32_t inv = (uint32_t)krt - 1u;
    unsigned char *q = smem;
    int *RSZ = reinterpret_cast<int *>(q); q += krt * 4;
    uint8_t *XR = q; q += bx64;
    uint32_t *PR = reinterpret_cast<uint32_t *>(q); if (kPriced) q += bx64 * 4;
    int *PG = reinterpret_cast<int *>(q); if (kPriced) q += krt * 4;
    uint32_t *BW = reinterpret_cast<uint32_t *>(q); if (hbw) q += bx64 * 4;
    WaveLds<NW> L;
    L.C = reinterpret_cast<uint32_t *>(q); q += bx64 * 4;
    L.K = reinterpret_cast<int *>(q); q += krt * 4;
    L.W = nullptr; L.RT = nullptr;
    int *KW = reinterpret_cast<int *>(q); q += kInitWaves * krt * 4;   // every wavefront's own copy of the rack counts
    unsigned long long *BEST = reinterpret_cast<unsigned long long *>(q);   // the hole's winner over the wavefronts (LDS atomic min), three in rotation

    for (int r = tid; r < krt; r += nthr) {
        RSZ[r] = r < T.R ? pl.rsz_pool[TD->rsz_off + r] : 0;
        if (kPriced) PG[r] = r < T.R ? price_units(pl.price_pool[TD->price_off + 2 * TD->B + r], prm.obj_scale) : 0;
    }
    __syncthreads();
    for (int x = tid; x < ((T.Bx + 63) & ~63); x += nthr) {
        const uint32_t r = mulhi((uint32_t)x, T.magic);
        const bool valid = x < T.Bx && (int)((uint32_t)x - r * (uint32_t)T.m) < RSZ[r < (uint32_t)krt ? r : 0];
        XR[x] = valid ? (uint8_t)r : (uint8_t)inv;
        if (kPriced) {
            uint32_t pr = 0;
            if (valid) {
                const int32_t *pp = pl.price_pool + TD->price_off;
                const int b = pl.ext_pool[TD->ext_off + x];
                pr = ((uint32_t)price_units(pp[b], prm.obj_scale) & 0xFFFFu) | ((uint32_t)price_units(pp[TD->B + b], prm.obj_scale) << 16);
            }
            PR[x] = pr;
            if (hbw) BW[x] = (valid && TD->has_bw) ? pl.bw_pool[TD->bw_off + x] : 0u;
        }
    }
    const Part<NW> *CUR = reinterpret_cast<const Part<NW> *>(pl.cur_pool + TD->cur_off);
    L.A = reinterpret_cast<Part<NW> *>(pl.state_pool + TD->state_off) + (uint64_t)rho * T.P;
    const uint32_t slo = TD->seed_lo, shi = TD->seed_hi;
    const int S = prm.obj_scale;
    for (int p = tid; p < T.P; p += nthr) {   // surviving current replicas stay in their slots
        Part<NW> c = CUR[p];
#pragma unroll
        for (int k = 1; k < NW; ++k)
            if (k >= T.RF) c.w[k] = kNoneW;
        L.A[p] = c;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    recount(T, L, tid, nthr, krt);
    __syncthreads();
    // Who reads what during the fill: C[x] only the wavefront that scans x's round, K[r] every wavefront.  So the winner's C entry is
    // bumped by the wavefront that owns it, the rack counts live in one copy per wavefront, and a hole costs ONE workgroup barrier.
    if (n_waves > 1) {
        for (int r = lane; r < krt; r += 64) KW[wave * krt + r] = L.K[r];
        L.K = KW + wave * krt;
        if (tid < 3) BEST[tid] = ~0ull;
        __syncthreads();
    }

    const uint32_t *HL = pl.cur_pool + TD->hole_off;
    const int n_rounds = (T.Bx + 63) >> 6;
    int par = 0;   // which BEST this hole uses
    for (int pass = 0; pass < 2; ++pass) {   // leader holes of all partitions first, then follower holes
        const uint32_t n_holes = HL[pass], *hl = HL + 2 + (pass ? HL[0] : 0u);
        // The rows of 64 holes are fetched at once, one hole per lane, and handed out by v_readlane: a pass lists every partition once, so
        // no row of the batch is written before its turn.  (Fetching them one hole ahead left two dependent global round trips, list entry
        // then row, per hole: 1.5 us, the whole fill once the scan was spread over the workgroup.)
        for (uint32_t h0 = 0; h0 < n_holes; h0 += 64) {
          const uint32_t nb = min(64u, n_holes - h0);
          const uint32_t p_l = hl[h0 + ((uint32_t)lane < nb ? (uint32_t)lane : 0u)];
          const Part<NW> a_l = L.A[p_l], c_l = CUR[p_l];
          for (uint32_t hi = 0; hi < nb; ++hi) {
            const int p = __builtin_amdgcn_readlane((int)p_l, (int)hi);
            Part<NW> a, c;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                a.w[w] = (uint32_t)__builtin_amdgcn_readlane((int)a_l.w[w], (int)hi);
                c.w[w] = (uint32_t)__builtin_amdgcn_readlane((int)c_l.w[w], (int)hi);
            }
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                if (k >= T.RF) break;
                if ((k == 0) != (pass == 0)) continue;
                if (a.w[k] != kNoneW) continue;   // uniform over the workgroup
                const uint32_t hmix = slo ^ fmix32(shi + (uint32_t)rho * 0x9E3779B1u + (uint32_t)(p * NW + k) * 0x27D4EB2Fu + 0x5BD1E995u + prm.gen * 0x632BE5ABu);
                const int wl = k == 0 ? T.w00 : T.w01, wf = k == 0 ? T.w10 : T.w11;
                uint32_t key = kKeyNull, xw_l = kNoneW;
                for (int j = wave; j < n_rounds; j += n_waves) {
                    const uint32_t x = (uint32_t)(j * 64 + lane);
                    const uint32_t r = XR[x];
                    const uint32_t xw = x | (r << 16);
                    const bool okx = (r != inv) & !in4(a, xw);
                    const uint32_t cn = L.C[x];
                    int dV = dinc((int)(cn & 0xFFFFu), T.rep_lo, T.rep_hi) + dinc(L.K[r], T.rack_lo, T.rack_hi) +
                             dinc(cnt4(a, r), T.prack_lo, T.prack_hi);
                    if (k == 0) dV += dinc((int)(cn >> 16), T.lead_lo, T.lead_hi);
                    const uint32_t tie = fmix32(hmix + x * 0x165667B1u) >> 24;
                    uint32_t keyx;
                    if (kPriced) {
                        const uint32_t prx = PR[x];
                        int dP = p_in((int)(cn & 0xFFFFu), T.rep_lo, T.rep_hi, price_rep(prx)) + p_in(L.K[r], T.rack_lo, T.rack_hi, PG[r]);
                        if (k == 0) dP += p_in((int)(cn >> 16), T.lead_lo, T.lead_hi, price_lead(prx));
                        keyx = okx ? make_key_tie_p(prm.lam_max, S, dV, role_w2(c, xw, wl, wf) + (hbw ? bw_of(BW[x], k == 0) : 0), dP, tie) : kKeyNull;
                    }
                    else keyx = okx ? make_key_tie(prm.lam_max, S, dV, role_w2(c, xw, wl, wf), tie) : kKeyNull;
                    if (keyx < key) { key = keyx; xw_l = xw; }   // (equal keys: the earlier round stays)
                }
                // this wavefront's winner: lowest key, then lowest lane (then, inside the lane, the earliest round: above)
                uint32_t kmin = wave_umin(key);
                const unsigned long long bal = __ballot(key == kmin);
                const int l_win = __ffsll((long long)bal) - 1;
                uint32_t xw_win = (uint32_t)__builtin_amdgcn_readlane((int)xw_l, l_win);
                if (n_waves > 1) {
                    // across the wavefronts the same order, (key, lane, round), packed with the rack into one 64-bit word: LDS atomic min.
                    // Three words in rotation: the one two holes ahead is reset behind this hole's barrier (everybody has read it before).
                    if (lane == 0) atomicMin(&BEST[par], ((unsigned long long)kmin << 32) | ((unsigned long long)l_win << 24) | ((unsigned long long)((xw_win & 0xFFFFu) >> 6) << 8) | (xw_win >> 16 & 0xFFu));
                    // LDS traffic only is ordered here: __syncthreads() would also wait for the winner's global store of the previous hole
                    // (vmcnt(0): a round trip to L2 per hole, ~1 us -- it was most of the fill); nobody reads those rows before the pass ends
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                    const unsigned long long bw = BEST[par];
                    const int nxt = par == 2 ? 0 : par + 1;
                    if (tid == 0) BEST[nxt == 2 ? 0 : nxt + 1] = ~0ull;
                    par = nxt;
                    const uint32_t lo = (uint32_t)bw;
                    xw_win = (((lo >> 8) & 0xFFFFu) << 6 | (lo >> 24)) | ((lo & 0xFFu) << 16);
                }
                a.w[k] = xw_win;
                if (lane == 0) {
                    const int owner = (int)(((xw_win & 0xFFFFu) >> 6) & (uint32_t)(n_waves - 1));   // (W is a power of two)
                    if (wave == owner) {
                        reinterpret_cast<uint32_t *>(&L.A[p])[k] = xw_win;
                        L.C[xw_win & 0xFFFFu] += (k == 0) ? 0x10001u : 1u;
                    }
                    L.K[xw_win >> 16] += 1;   // own copy
                }
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // pass 1 reads the rows pass 0 wrote
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------------
// the "LDS carve" of search_body, summed (pinned below)
constexpr size_t search_lds_total(size_t maxP, size_t maxBx, size_t waves, bool global_a, bool priced, size_t nw, bool bw, int maxR, size_t team, bool cur_global) {
    const size_t a = global_a ? 0 : maxP * 4 * nw, bx64 = (maxBx + 63) & ~(size_t)63, krt = (size_t)search_rack_tab(maxR);
    const size_t shared = (cur_global ? 0 : a) + krt * 4 + bx64 + (priced ? (bw ? 2 : 1) * bx64 * 4 + krt * 4 : 0);
    if (team > 0)   // one set of counters / band states / rack totals, one RT per wavefront, the proposal records, the partial sums
        return shared + bx64 * 6 + krt * 4 + team * krt * 4 + 2 * 16 * kTeamRec * 4 + 16 * 2 * 4;
    return shared + waves * (a + bx64 * 6 + krt * 8);
}
size_t search_lds_bytes(int maxP, int maxBx, int waves, bool global_a, bool priced, int nw, bool bw, int maxR, int team, bool cur_global) {
    return search_lds_total((size_t)maxP, (size_t)maxBx, (size_t)waves, global_a, priced, (size_t)nw, bw, maxR, (size_t)team, cur_global);
}
// config 4 (50 partitions, RF 3, 500 brokers on 10 racks, 4 wavefronts); the same with 8 words per partition; priced, and with broker weights;
// working words only (k_search_curg) at 9,800 partitions; a team of 8 on a topic in global memory
static_assert(search_lds_total(50, 500, 4, false, false, 4, false, 10, 0, false) == 19104 && search_lds_total(50, 500, 4, false, false, 8, false, 10, 0, false) == 23104 &&
              search_lds_total(50, 500, 4, false, true, 4, false, 10, 0, false) == 21408 && search_lds_total(50, 500, 4, false, true, 4, true, 10, 0, false) == 23456 &&
              search_lds_total(9800, 500, 1, false, false, 4, false, 10, 0, true) == 161152 && search_lds_total(100000, 500, 1, true, false, 4, false, 10, 8, false) == 7808,
              "search_lds_total no longer sums the LDS carve of search_body");

bool search_rf3_eligible(bool global_a, bool cur_global, bool priced, int nw, int team) { return !global_a && !cur_global && !priced && nw == 4 && team == 0; }

// The "small cost" property of a launch: no cost the kernel forms can leave int16, so the clamp to +-32768 in key_of and in the scans
// changes nothing and two costs fit the halves of one register (search_body, kSmall).  Costs are lam * dV - S * dObj with
// lam_min <= lam <= lam_max, S = obj_scale, and w = the largest |w00..w11| over the topics of the launch group.
//   |dV|: every row a move touches changes its band violation by -1, 0 or +1 (dinc / ddec), so |dV| <= rows touched.
//     REPLACE (p,k) u -> x : replica rows of u and x (2), their leader rows when k = 0 (2), the rack totals of both racks (2), the
//                            partition's counts in both racks (2)                                                    -> |dV| <= 8
//     EXCHANGE (p,k) <-> (q,j): leader rows of u and v (2), each partition's counts in both racks (4)             -> |dV| <= 6
//     LEADER-SWAP            : leader rows of the two brokers                                                      -> |dV| <= 2
//     tournament score       : a part of a REPLACE's (at most 4 rows) or of an EXCHANGE's (2)                      -> |sc| <= 4
//   |dObj|: a sum of role weights with signs: REPLACE new - old (2 terms), EXCHANGE and LEADER-SWAP 4 terms, the tournament 1 -> <= 4 w
//   the scans: the constant K0 = S * g_old + lam * dV_old (|dV_old| <= 2) alone is within 2 lam + S w; a candidate adds lam * dVx with
//     |dVx| <= 6 (replica and leader row of x, 4 rows of racks) and subtracts S * weight: K0 + lam * dVx - S * w within 8 lam + 2 S w
//   So every cost, and every partial sum a packed instruction forms on the way, is within 8 lam_max + 4 S w.  The rule admits half of
//   int16's range, kSmallCostMax = 16384: the biased cost field then stays inside [16384, 49152], far from both the clamp's ends and
//   the no-candidate value 0xFFFF.  (The default options give 8 * 40 + 4 * 4 * 4 = 384.)
// False whenever the launch is priced (prices are added to the cost; broker weights make a session priced).
// The small-cost form also looks a broker's band rows up in per-topic tables (band_tab, kao_search_dev.h): a launch group takes it
// only when the replica and the leader band of every topic fit one (hi - lo <= 2; a balanced topic has hi - lo <= 1, wider bands come
// from bounds_override), so the kernel holds one form of the row, chosen per launch on the host.
bool search_band_tabs(int rep_lo, int rep_hi, int lead_lo, int lead_hi) { return band_tab_fits(rep_lo, rep_hi) && band_tab_fits(lead_lo, lead_hi); }
bool search_small_cost(int lam_min, int lam_max, int obj_scale, int w_abs_max, bool priced) {
    if (priced || lam_min < 0 || lam_max < lam_min || obj_scale < 1 || w_abs_max < 0) return false;
    return 8 * (int64_t)lam_max + 4 * (int64_t)obj_scale * (int64_t)w_abs_max <= (int64_t)kSmallCostMax;
}

// The K-search kernel for a launch group, chosen in ONE place for the launch and for the occupancy query: f is called with the kernel
// as a compile-time constant (launch_lds keeps its per-kernel state by it).  rft = 3: every topic RF 3, at most 3 current replicas
// (kao_session.cpp); small: search_small_cost of the launch's options and the group's weights; chunked: one workgroup per ticket
// (search_chunk_eligible groups only).
using SearchKernel = void (*)(SearchPools, SearchParams);
template <SearchKernel kKernel> using KernelConst = std::integral_constant<SearchKernel, kKernel>;
template <class F>
static void with_search_kernel(bool global_a, bool curg, int team, bool priced, int nw, bool wide, int rft, bool small, bool chunked, F f) {
    chunked = chunked && search_chunk_eligible(global_a, curg, team);
    if (rft == 3 && search_rf3_eligible(global_a, curg, priced, nw, team)) {
        if (chunked) {
            if (small) { if (wide) f(KernelConst<k_search_chunked<false, 4, true, 3, true>>{}); else f(KernelConst<k_search_chunked<false, 4, false, 3, true>>{}); }
            else if (wide) f(KernelConst<k_search_chunked<false, 4, true, 3>>{});
            else f(KernelConst<k_search_chunked<false, 4, false, 3>>{});
        }
        else if (small) { if (wide) f(KernelConst<k_search<false, false, 4, true, 3, true>>{}); else f(KernelConst<k_search<false, false, 4, false, 3, true>>{}); }
        else if (wide) f(KernelConst<k_search<false, false, 4, true, 3>>{});
        else f(KernelConst<k_search<false, false, 4, false, 3>>{});
        return;
    }
    with_flags(priced, nw == 8, [&](auto p, auto k8) {
        constexpr bool kPriced = decltype(p)::value;
        constexpr int NW = decltype(k8)::value ? 8 : 4;
        if (curg) f(KernelConst<k_search_curg<kPriced, NW>>{});          // working assignment in LDS, current assignment from L2
        else if (team > 0) f(KernelConst<k_team<kPriced, NW>>{});        // (topics in global memory only)
        else if (global_a) f(KernelConst<k_search<true, kPriced, NW, true>>{});   // (topics in global memory are always wide)
        else if (chunked) { if (wide) f(KernelConst<k_search_chunked<kPriced, NW, true>>{}); else f(KernelConst<k_search_chunked<kPriced, NW, false>>{}); }
        else if (wide) f(KernelConst<k_search<false, kPriced, NW, true>>{});
        else f(KernelConst<k_search<false, kPriced, NW, false>>{});
    });
}

void launch_search(const SearchPools &pools, const SearchParams &prm, int n_blocks, int waves, bool global_a, bool priced, int nw, void *stream, int team, int rft, bool small) {
    const bool curg = prm.cur_global != 0 && !global_a, wide = prm.wide != 0;
    const size_t lds = search_lds_bytes(prm.maxP, prm.maxBx, waves, global_a, priced, nw, prm.bw != 0, prm.maxR, team, curg);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(n_blocks), block(64 * (team > 0 && !curg ? team : waves));   // a team: one workgroup per restart, `team` wavefronts each; a chunked launch: one per ticket
    with_search_kernel(global_a, curg, team, priced, nw, wide, rft, small, prm.chunks != 0, [&](auto k) {
        launch_lds<decltype(k)::value>(grid, block, lds, st, pools, prm);
    });
}

// Workgroups per compute unit of the kernel a chunked launch of these flags runs, from the runtime's occupancy query for its block size
// and LDS carve.
int search_resident_blocks(int waves, bool priced, int nw, bool wide, int rft, bool small, size_t lds) {
    // (asked at every session creation that might chunk; the runtime's query costs a few tenths of a millisecond, which a solve of two
    //  milliseconds would notice: the answer per kernel, block size, LDS carve and device is kept)
    static std::mutex mu;
    static std::map<std::tuple<const void *, int, size_t, int>, int> known;
    int n = 0, dev = 0;
    (void)hipGetDevice(&dev);
    with_search_kernel(false, false, 0, priced, nw, wide, rft, small, true, [&](auto k) {
        const void *fn = reinterpret_cast<const void *>(decltype(k)::value);
        const auto key = std::make_tuple(fn, 64 * waves, lds, dev);
        std::lock_guard<std::mutex> lock(mu);
        const auto it = known.find(key);
        if (it != known.end()) { n = it->second; return; }
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 64 * waves, lds) != hipSuccess) { (void)hipGetLastError(); n = 0; return; }
        known[key] = n;
    });
    return n;
}

// K-init for one launch group of topics in global memory: `n_blocks` block-map entries of `per_block` restarts each, `waves` wavefronts per
// restart (0 = automatic).  False when the tables do not fit (the caller leaves prm.init = 1: k_search fills the holes itself).
bool launch_init(const SearchPools &pools, const SearchParams &prm, int n_blocks, int per_block, bool priced, int nw, int waves, void *stream) {
    const size_t lds = init_lds_bytes(prm.maxBx, prm.maxR, priced, prm.bw != 0);
    if (lds > 160 * 1024) return false;
    // (config 5 as one topic, 15,000 holes x 16 rounds, per K-init: 59.2 / 21.8 / 17.3 / 18.0 ms with 1 / 4 / 8 / 16 wavefronts -- beyond two rounds
    // per wavefront the hole's fixed part, ~200 instructions of reduce / exchange / update behind one another, is what is left)
    waves = waves > 0 ? std::min(kInitWaves, waves) : std::min(8, std::max(1, (prm.maxBx + 63) / 64));
    while (waves & (waves - 1)) waves &= waves - 1;   // a power of two (the kernel's owner-of-a-round mask)
    const dim3 grid((unsigned)(n_blocks * per_block)), block((unsigned)(64 * waves));
    with_flags(priced, nw == 8, [&](auto p, auto k8) {
        launch_lds<k_init<decltype(p)::value, decltype(k8)::value ? 8 : 4>>(grid, block, lds, static_cast<hipStream_t>(stream), pools, prm, per_block);
    });
    return true;
}

}  // namespace kao

// Test hooks (include/kao.h): the band-row and C7 lookups on the host, through the table builders the kernels use.
extern "C" int kao_search_band_row(int32_t lo, int32_t hi, int32_t c, int32_t force_plain, int32_t *fits) {
    using namespace kao;
    const bool tab = band_tab_fits(lo, hi);
    if (fits) *fits = tab ? 1 : 0;
    if (tab && !force_plain) return (int)band_lookup_plain(c, band_tab_bias(lo), band_tab(lo, hi));
    const int a = std::min(std::max(c - lo, -1), 1), b = std::min(std::max(c - hi, -1), 1);   // band_entry: the two clamps, 3 a + b, the shift
    return (int)((kBandTab >> (uint32_t)(6 * (3 * a + b) + 24)) & 63u);
}
extern "C" int kao_search_rack_delta(int32_t lo, int32_t hi, int32_t c, int32_t dec) {
    const uint32_t tab = kao::c7_tab(dec != 0, lo, hi);
    const uint32_t f = (tab >> ((2u * (uint32_t)c) & 31u)) & 3u;   // v_bfe_i32 at twice the count, two bits, sign-extended
    return (int)(f ^ 2u) - 2;
}
