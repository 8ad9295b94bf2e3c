// kao_canon.hip -- K-canon (gfx950): the canonical tie-break of kao_canonicalize on the device, and its launcher.
#include "kao_search_dev.h"

namespace kao {

// ------------------------------------------------------------------------------------------------
// K-canon: canonical tie-break among equal-objective feasible assignments (kao_canonicalize)
// ------------------------------------------------------------------------------------------------
// Scanning partitions and slots in order, every NEWLY placed replica (its broker is not a current replica of the
// partition) moves to the lowest DENSE broker index that keeps the assignment feasible; repeated to a fixpoint.
// Such a move never changes the objective (neither broker carries weight on that partition) and, the state being
// feasible, it stays feasible iff the move's violation delta is 0 -- so this is the REPLACE scan of k_search with
// "delta == 0" as the filter and the dense index as the key.  One wavefront; the assignment and current-assignment
// words stay in global memory (any topic size); broker / rack tables in LDS.  status = {input feasible, #moves}.
template <int NW>
__global__ __launch_bounds__(64) void k_canon(const TopicDev *TD, const Part<NW> *cur_words, const uint16_t *ext, const int32_t *rsz,
                                              Part<NW> *A, int maxBx, int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const TopicRegs T = topic_regs(TD);
    const int bx64 = (maxBx + 63) & ~63;   // LDS: [RSZ int[kRackTab]] [XR u8[bx64]] [C u32[bx64]] [K int[kRackTab]] (canon_lds_total)
    int *RSZ = reinterpret_cast<int *>(smem);
    uint8_t *XR = smem + kRackTab * 4;
    WaveLds<NW> L;
    L.A = A;
    L.C = reinterpret_cast<uint32_t *>(smem + kRackTab * 4 + bx64);
    L.K = reinterpret_cast<int *>(smem + kRackTab * 4 + bx64 + bx64 * 4);
    L.RT = L.K;  // unused here
    L.W = reinterpret_cast<uint16_t *>(L.C);   // unused here
    // (the staging of search_body, with an entry for every rack: the padding marker is 0xFF)
    for (int r = lane; r < kRackTab; r += 64) RSZ[r] = r < T.R ? rsz[r] : 0;
    __syncthreads();
    for (int x = lane; x < ((T.Bx + 63) & ~63); x += 64) {
        const uint32_t r = mulhi((uint32_t)x, T.magic);
        XR[x] = (x < T.Bx && (int)((uint32_t)x - r * (uint32_t)T.m) < RSZ[r < (uint32_t)kRackTab ? r : 0]) ? (uint8_t)r : (uint8_t)0xFF;
    }
    __syncthreads();
    recount(T, L, lane, 64, kRackTab);
    int V, obj;
    full_cost(T, L, cur_words, RSZ, lane, 64, V, obj);
    if (V != 0) {  // only feasible assignments are polished
        if (lane == 0) { status[0] = 0; status[1] = 0; }
        return;
    }
    int moves = 0;
    bool changed = true;
    while (changed) {
        changed = false;
        for (int pbase = 0; pbase < T.P; pbase += 64) {
            bool has_new = false;
            if (pbase + lane < T.P) {
                const Part<NW> al = L.A[pbase + lane];
                const Part<NW> cl = cur_words[pbase + lane];
#pragma unroll
                for (int k = 0; k < NW; ++k) has_new |= (k < T.RF) & !in4(cl, al.w[k]);
            }
            unsigned long long todo = __ballot(has_new);
            while (todo) {
                const int p = pbase + __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                Part<NW> a = L.A[p];
                const Part<NW> c = cur_words[p];
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    if (k >= T.RF) break;
                    const uint32_t uw = a.w[k];
                    if (in4(c, uw)) continue;  // a retained current replica stays where it is (wave-uniform)
                    const uint32_t old_dense = ext[uw & 0xFFFFu];
                    const uint32_t ro = uw >> 16;
                    const bool lead = k == 0;
                    const uint32_t co = L.C[uw & 0xFFFFu];
                    int dV_old = ddec((int)(co & 0xFFFFu), T.rep_lo, T.rep_hi);
                    if (lead) dV_old += ddec((int)(co >> 16), T.lead_lo, T.lead_hi);
                    const int dV_rack_old = ddec(L.K[ro], T.rack_lo, T.rack_hi) + ddec(cnt4(a, ro), T.prack_lo, T.prack_hi);
                    uint32_t key = kKeyNull;
                    for (int base = 0; base < T.Bx; base += 64) {
                        const uint32_t x = (uint32_t)(base + lane);
                        const uint32_t r = XR[x];
                        const uint32_t xw = x | (r << 16);
                        bool ok = (r != 0xFFu) && !in4(a, xw) && !in4(c, xw);
                        const uint32_t dense = ok ? (uint32_t)ext[x] : 0xFFFFu;
                        ok = ok & (dense < old_dense);
                        const uint32_t cn = L.C[x];
                        int dV = dV_old + dinc((int)(cn & 0xFFFFu), T.rep_lo, T.rep_hi);
                        if (lead) dV += dinc((int)(cn >> 16), T.lead_lo, T.lead_hi);
                        if (r != ro) dV += dV_rack_old + dinc(L.K[r & 255u], T.rack_lo, T.rack_hi) + dinc(cnt4(a, r), T.prack_lo, T.prack_hi);
                        const uint32_t kx = (ok & (dV == 0)) ? ((dense << 16) | x) : kKeyNull;
                        key = min(key, kx);
                    }
                    const uint32_t kmin = wave_umin(key);
                    if (kmin == kKeyNull) continue;
                    const uint32_t xn = kmin & 0xFFFFu;
                    const uint32_t rn = XR[xn];
                    const uint32_t xw_new = xn | (rn << 16);
                    a.w[k] = xw_new;
                    if (lane == 0) {
                        const uint32_t d = lead ? 0x10001u : 1u;
                        reinterpret_cast<uint32_t *>(&L.A[p])[k] = xw_new;
                        L.C[uw & 0xFFFFu] -= d;
                        L.C[xn] += d;
                        L.K[ro] -= 1;
                        L.K[rn] += 1;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                    changed = true;
                    ++moves;
                }
            }
        }
    }
    if (lane == 0) { status[0] = 1; status[1] = moves; }
}

// the carve at the top of k_canon, summed (pinned below)
constexpr size_t canon_lds_total(size_t maxBx) {
    const size_t bx64 = (maxBx + 63) & ~(size_t)63;
    return kRackTab * 4 + bx64 + bx64 * 4 + kRackTab * 4;
}
size_t canon_lds_bytes(int maxBx) { return canon_lds_total((size_t)maxBx); }
static_assert(canon_lds_total(500) == 4608 && canon_lds_total(65535) == 329728, "canon_lds_total no longer sums the LDS carve of k_canon");

void launch_canon(const TopicDev *topic, const uint32_t *cur_words, const uint16_t *ext, const int32_t *rsz, uint32_t *A, int maxBx,
                  int nw, int32_t *status, void *stream) {
    const auto go = [&](auto k8) {
        constexpr int NW = decltype(k8)::value ? 8 : 4;
        launch_lds<k_canon<NW>>(dim3(1), dim3(64), canon_lds_bytes(maxBx), static_cast<hipStream_t>(stream), topic, reinterpret_cast<const Part<NW> *>(cur_words), ext,
                                rsz, reinterpret_cast<Part<NW> *>(A), maxBx, status);
    };
    if (nw == 8) go(std::true_type{}); else go(std::false_type{});
}

}  // namespace kao
