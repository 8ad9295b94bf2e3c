// kao_failover.hip -- kao_failover_order: the follower order that keeps the peak leader count after a broker or rack failure as low
// as it can be, with the fewest follower swaps.  Kernels and the C entry point.
//
// Kafka hands an orphaned partition to the first live replica of its list, so for the failure scenario g that takes the preferred
// leader of p down, the slot e(p) = the first eligible follower inherits p.  Choosing another eligible slot j(p) and swapping it
// with e(p) moves no data.  For a cap M on every surviving broker's leaders, scenario g is a min-cost flow: each affected partition
// sends one unit to a broker of an eligible slot (cost 0 for e(p), 1 otherwise), broker b takes at most M - lead[b] units.
// (the first and the third kernel, the host function that runs the three and the host-side checks live in kao_failover_dev.h, shared
// with kao_wfailover.hip; the second in kao_plan_dev.h)
//   k_fo_classify  one pass over the partitions: lead[], the scenario of p, its eligible slots, e(p), the scenarios' sizes
//   k_bucket_offsets  exclusive scan of the sizes (one workgroup)
//   k_fo_scatter   the affected partitions bucketed by scenario (counting sort; the order inside a bucket is not used)
//   k_fo_solve     ONE WORKGROUP PER SCENARIO, all scenarios in one launch: bisection on M between the lower end
//                  max(max lead, ceil(leaders left / brokers left)) and peak_before, every probe a max-flow from the start state
//                  j = e, then one min-cost solve at peak_after, then the swaps
// A solve at cap M is successive shortest paths as in kao_leaders.hip (but with 32-bit keys in LDS, below: not the 64-bit flow keys
// of kao_plan_dev.h), on the residual graph whose arcs are never stored: partition
// p on slot c = cur[p] gives rows[p][c] -> rows[p][j] for every other eligible slot j, cost -1 when j == e(p), +1 when c == e(p),
// 0 otherwise (all 0 in a probe).  room[b] = M - lead[b] - inherit(b): negative = excess (sources), positive = free capacity.
// A PHASE:
//   1. keys (distance, arcs on the path) of every broker from the sources by Jacobi rounds over all arcs until a round changes
//      nothing; a key is (distance + 2^14) << 16 | arcs in 32 bits, minimised as one word.  Round r reads buffer r & 1 and
//      atomicMins into the other one, every node bidding its own key too, so the round count is a function of the input.
//   2. every tight arc bids its GLOBAL slot id p * width + j into pred[head]: the lowest id wins, whatever the bucket order.
//   3. the brokers with room at the smallest distance dmin (their arcs to the sink are the tight ones) are marked in a bitmap; one
//      lane walks them in index order and augments each one's predecessor path while it uses no partition an earlier path of this
//      phase used and starts at a broker that still has excess.  All those paths consist of tight arcs, so the keys stay feasible
//      potentials and the pseudoflow stays optimal for its imbalances.  The first target always gets its path, so a phase without
//      a reachable broker with room proves M infeasible.
// M is never raised inside a running solve (a newly opened sink arc could close a negative cycle with the -1 arcs): every probe
// starts over from j = e.  Node state (two key buffers, pred, room, the bitmap) lives in dynamic LDS, 16.125 bytes per broker.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "kao_failover_dev.h"

namespace {

constexpr uint32_t kFoInf = 0xFFFFFFFFu;
constexpr uint32_t kFoSource = 1u << 30;   // distance 0, no arc
constexpr uint32_t kFoNoPred = 0xFFFFFFFFu;
enum { SH_FLAG = 0, SH_LEFT = 1, SH_DMIN = 2, SH_AUG = 3, SH_MAXLEN = 4, SH_MAXLEAD = 5, SH_SUMLEAD = 6, SH_ALIVE = 7, SH_PEAK = 8,
       SH_CNT = 9, SH_ERR = 10, SH_N = 16 };

// tail, head and cost of the arc of local slot i of the scenario (partition list[i / W], slot i % W); false when there is none
__device__ __forceinline__ bool fo_arc(int i, int W, bool costed, const int32_t *__restrict__ list, const uint16_t *__restrict__ rows,
                                       const uint16_t *__restrict__ meta, const uint8_t *cur, int &u, int &v, int &c, uint32_t &id) {
    const int q = i / W, j = i - q * W, p = list[q], m = meta[p], c0 = cur[p];
    if (j == c0 || !((m >> (8 + j)) & 1)) return false;
    const int e = m & 0xFF;
    u = rows[(size_t)p * W + c0];
    v = rows[(size_t)p * W + j];
    c = !costed ? 0 : (j == e ? -1 : (c0 == e ? 1 : 0));
    id = (uint32_t)p * (uint32_t)W + (uint32_t)j;
    return true;
}

__device__ __forceinline__ uint32_t fo_step(uint32_t ku, int c) { return ku + ((uint32_t)c << 16) + 1u; }

// Step 3 of a phase, one lane.  Returns the paths augmented.
__device__ __forceinline__ int fo_extract(int B, int W, int32_t stamp, const uint16_t *__restrict__ rows, uint8_t *cur,
                                          int32_t *claim, const uint32_t *K, const uint32_t *pred, int32_t *room, const uint32_t *bits,
                                          int32_t *maxlen) {
    int naug = 0;
    for (int w = 0; w < (B + 31) / 32; ++w) {
        uint32_t word = bits[w];
        while (word) {
            const int t = w * 32 + __ffs((int)word) - 1;
            word &= word - 1;
            while (room[t] > 0) {
                bool ok = true;
                int v = t, steps = 0;
                while ((K[v] & 0xFFFFu) != 0u) {   // arcs on the way here: 0 at the path's first node
                    const uint32_t a = pred[v];
                    if (a == kFoNoPred || ++steps > B) { ok = false; break; }
                    const int p = (int)(a / (uint32_t)W);
                    if (claim[p] == stamp) { ok = false; break; }
                    v = rows[(size_t)p * W + cur[p]];
                }
                if (!ok || room[v] >= 0) break;
                const int src = v;
                v = t;
                while ((K[v] & 0xFFFFu) != 0u) {
                    const uint32_t a = pred[v];
                    const int p = (int)(a / (uint32_t)W);
                    v = rows[(size_t)p * W + cur[p]];
                    cur[p] = (uint8_t)(a - (uint32_t)p * (uint32_t)W);
                    claim[p] = stamp;
                }
                room[src] += 1;
                room[t] -= 1;
                ++naug;
                *maxlen = max(*maxlen, (int32_t)(K[t] & 0xFFFFu));
            }
        }
    }
    return naug;
}

// ---- one scenario per workgroup ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFoSoloLarge) void k_fo_solve(int B, int W, int scope, int dry_run, uint16_t *__restrict__ rows,
                                                           const uint8_t *__restrict__ rack_of, const int32_t *__restrict__ lead,
                                                           const uint16_t *__restrict__ meta, uint8_t *__restrict__ cur,
                                                           int32_t *__restrict__ claim, const int32_t *__restrict__ cnt,
                                                           const int32_t *__restrict__ offl, const int32_t *__restrict__ start,
                                                           const int32_t *__restrict__ list_all, int32_t *__restrict__ scen,
                                                           int32_t *__restrict__ ctl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fo_smem[];
    __shared__ int32_t sh[SH_N];
    const int g = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, n = cnt[g], NS = n * W, NW = (B + 31) / 32;
    const int32_t *list = list_all + start[g];
    if (tid < SH_N) sh[tid] = 0;
    __syncthreads();
    // the surviving brokers: how many, their leaders, the most any of them leads
    {
        int mx = 0, sum = 0, alive = 0;
        for (int b = tid; b < B; b += NT)
            if (!fo_dead(b, g, scope, rack_of)) { mx = max(mx, lead[b]); sum += lead[b]; ++alive; }
        if (alive) { atomicMax(&sh[SH_MAXLEAD], mx); atomicAdd(&sh[SH_SUMLEAD], sum); atomicAdd(&sh[SH_ALIVE], alive); }
    }
    __syncthreads();
    if (n == 0) {   // nothing to choose: the peak is the survivors' largest leader count
        if (tid == 0) {
            int32_t *o = scen + 5 * (size_t)g;
            o[0] = 0; o[1] = offl[g]; o[2] = sh[SH_MAXLEAD]; o[3] = sh[SH_MAXLEAD]; o[4] = 0;
        }
        return;
    }
    uint32_t *key0 = reinterpret_cast<uint32_t *>(fo_smem), *key1 = key0 + B, *pred = key1 + B, *bits = pred + B + B;
    int32_t *room = reinterpret_cast<int32_t *>(pred + B);

    // peak_before: the start state j = e
    for (int b = tid; b < B; b += NT) room[b] = fo_dead(b, g, scope, rack_of) ? 0 : lead[b];
    __syncthreads();
    for (int q = tid; q < n; q += NT) { const int p = list[q]; atomicAdd(&room[rows[(size_t)p * W + (meta[p] & 0xFF)]], 1); }
    __syncthreads();
    {
        int mx = 0;
        for (int b = tid; b < B; b += NT) mx = max(mx, room[b]);
        if (mx) atomicMax(&sh[SH_PEAK], mx);
    }
    __syncthreads();
    int lo = max(sh[SH_MAXLEAD], (sh[SH_SUMLEAD] + n + sh[SH_ALIVE] - 1) / sh[SH_ALIVE]), hi = sh[SH_PEAK];
    const int peak_before = hi;
    int probes = 0, phases = 0, rounds = 0, paths = 0, stamp = 0;
    bool err = false;
    for (bool last = lo >= hi;; last = lo >= hi) {   // probes at (lo + hi) / 2 while lo < hi, then the min-cost solve at hi
        const int M = last ? hi : (lo + hi) / 2;
        const bool costed = last;
        ++probes;
        for (int b = tid; b < B; b += NT) room[b] = fo_dead(b, g, scope, rack_of) ? 0 : M - lead[b];
        if (tid == 0) sh[SH_LEFT] = 0;
        __syncthreads();
        for (int q = tid; q < n; q += NT) {
            const int p = list[q], e = meta[p] & 0xFF;
            cur[p] = (uint8_t)e;
            atomicSub(&room[rows[(size_t)p * W + e]], 1);
        }
        __syncthreads();
        {
            int ex = 0;
            for (int b = tid; b < B; b += NT) ex += max(-room[b], 0);
            if (ex) atomicAdd(&sh[SH_LEFT], ex);
        }
        __syncthreads();
        bool feasible = true;
        while (sh[SH_LEFT] > 0) {
            ++phases;
            ++stamp;
            for (int v = tid; v < B; v += NT) {
                const uint32_t k = room[v] < 0 ? kFoSource : kFoInf;
                key0[v] = k;
                key1[v] = k;
                pred[v] = kFoNoPred;
            }
            for (int w = tid; w < NW; w += NT) bits[w] = 0u;
            if (tid == 0) { sh[SH_DMIN] = 0x7FFFFFFF; sh[SH_AUG] = 0; }
            __syncthreads();
            for (int r = 0;; ++r) {
                if (tid == 0) sh[SH_FLAG] = 0;
                __syncthreads();
                const uint32_t *X = (r & 1) ? key1 : key0;
                uint32_t *Y = (r & 1) ? key0 : key1;
                bool ch = false;
                for (int i = tid; i < NS; i += NT) {
                    int u, v, c;
                    uint32_t id;
                    if (!fo_arc(i, W, costed, list, rows, meta, cur, u, v, c, id)) continue;
                    const uint32_t ku = X[u];
                    if (ku == kFoInf) continue;
                    const uint32_t nk = fo_step(ku, c);
                    if (nk < X[v]) { atomicMin(&Y[v], nk); ch = true; }
                }
                for (int v = tid; v < B; v += NT) {
                    const uint32_t kv = X[v];
                    if (kv != kFoInf) atomicMin(&Y[v], kv);
                }
                if (ch) sh[SH_FLAG] = 1;
                __syncthreads();
                ++rounds;
                const bool any = sh[SH_FLAG] != 0;
                __syncthreads();
                if (!any) break;
                if (r > B) {   // cannot happen (no negative cycle: keys settle within B rounds); the host stops on it
                    if (tid == 0) sh[SH_ERR] = 1;
                    break;
                }
            }
            __syncthreads();
            if (sh[SH_ERR]) { err = true; break; }
            // the settled keys are in both buffers; targets = brokers with room at the smallest distance
            for (int v = tid; v < B; v += NT)
                if (room[v] > 0 && key0[v] != kFoInf) atomicMin(&sh[SH_DMIN], (int32_t)(key0[v] >> 16));
            for (int i = tid; i < NS; i += NT) {
                int u, v, c;
                uint32_t id;
                if (!fo_arc(i, W, costed, list, rows, meta, cur, u, v, c, id)) continue;
                const uint32_t ku = key0[u];
                if (ku != kFoInf && fo_step(ku, c) == key0[v]) atomicMin(&pred[v], id);
            }
            __syncthreads();
            const int dmin = sh[SH_DMIN];
            if (dmin == 0x7FFFFFFF) { feasible = false; break; }   // (uniform: read after the barrier, written before it)
            for (int v = tid; v < B; v += NT)
                if (room[v] > 0 && key0[v] != kFoInf && (int32_t)(key0[v] >> 16) == dmin) atomicOr(&bits[v >> 5], 1u << (v & 31));
            __syncthreads();
            if (tid == 0) {
                const int k = fo_extract(B, W, stamp, rows, cur, claim, key0, pred, room, bits, &sh[SH_MAXLEN]);
                sh[SH_AUG] = k;
                sh[SH_LEFT] -= k;
            }
            __syncthreads();
            const int k = sh[SH_AUG];
            paths += k;
            __syncthreads();
            if (k == 0) { err = true; break; }   // cannot happen: the first target always gets its path
        }
        __syncthreads();
        if (err || last) break;
        if (feasible) hi = M; else lo = M + 1;
    }
    // the result: peak_after from the loads themselves, the swaps
    if (tid == 0) { sh[SH_PEAK] = 0; sh[SH_CNT] = 0; }
    __syncthreads();
    {
        int mx = 0;
        for (int b = tid; b < B; b += NT)
            if (!fo_dead(b, g, scope, rack_of)) mx = max(mx, hi - room[b]);
        if (mx) atomicMax(&sh[SH_PEAK], mx);
        int moved = 0;
        for (int q = tid; q < n; q += NT) {
            const int p = list[q], e = meta[p] & 0xFF, c = cur[p];
            if (c == e) continue;
            ++moved;
            if (!dry_run && !err) {
                uint16_t *row = rows + (size_t)p * W;
                const uint16_t a = row[e], b = row[c];
                row[e] = b;
                row[c] = a;
            }
        }
        if (moved) atomicAdd(&sh[SH_CNT], moved);
    }
    __syncthreads();
    if (tid == 0) {
        int32_t *o = scen + 5 * (size_t)g;
        o[0] = n; o[1] = offl[g]; o[2] = peak_before; o[3] = sh[SH_PEAK]; o[4] = sh[SH_CNT];
        atomicAdd(&ctl[FS_SCEN], 1);
        atomicAdd(&ctl[FS_PROBES], probes);
        atomicAdd(&ctl[FS_PHASES], phases);
        atomicAdd(&ctl[FS_ROUNDS], rounds);
        atomicAdd(&ctl[FS_PATHS], paths);
        atomicMax(&ctl[FS_MAXLEN], sh[SH_MAXLEN]);
        atomicAdd(&ctl[FS_REORDERED], sh[SH_CNT]);
        if (err) atomicAdd(&ctl[FS_ERR], 1);
    }
}

}  // namespace

extern "C" int kao_failover_order(int32_t n_brokers, int32_t n_racks, const uint8_t *rack_of, int32_t n_partitions, int32_t width,
                                  uint16_t *rows, int32_t scope, int32_t dry_run, int32_t *scen, int32_t *n_reordered, int32_t stats[8]) {
    int rc = validate_failover("kao_failover_order: ", n_brokers, n_racks, rack_of, n_partitions, width, rows, scope, scen, n_reordered);
    if (rc) return rc;
    if ((rc = require_init())) return rc;
    const int B = n_brokers, P = n_partitions, W = width, G = scope == 0 ? n_brokers : n_racks;
    const size_t PW = (size_t)P * W;

    // one arena: ctl i32[FS_N] | lead i32[B] | cnt, off i32[G] (zeroed up to here) | start, fill i32[G] | scen i32[5G] | scen_of i32[P] |
    //            list i32[P] | claim i32[P] | rows u16[PW] | meta u16[P] | cur u8[P] | rack_of u8[B]
    Carve cv;
    const size_t o_ctl = cv.take<int32_t>(FS_N), o_lead = cv.take<int32_t>(B), o_cnt = cv.take<int32_t>(G), o_off = cv.take<int32_t>(G),
                 zeroed = cv.end(), o_start = cv.take<int32_t>(G), o_fill = cv.take<int32_t>(G), o_scen = cv.take<int32_t>(5 * (size_t)G),
                 o_sof = cv.take<int32_t>(P), o_list = cv.take<int32_t>(P), o_claim = cv.take<int32_t>(P), o_rows = cv.take<uint16_t>(PW),
                 o_meta = cv.take<uint16_t>(P), o_cur = cv.take<uint8_t>(P), o_rack = cv.take<uint8_t>(B);
    CallBufs m;
    if ((rc = m.open(cv.end()))) return rc;
    hipStream_t st = m.stream;
    const FoScen d{m.at<int32_t>(o_lead), m.at<int32_t>(o_sof), m.at<int32_t>(o_cnt), m.at<int32_t>(o_off), m.at<int32_t>(o_start), m.at<int32_t>(o_fill),
                   m.at<int32_t>(o_list), m.at<int32_t>(o_claim), m.at<int32_t>(o_ctl), m.at<uint16_t>(o_meta), m.at<uint8_t>(o_cur)};
    int32_t *d_scen = m.at<int32_t>(o_scen);
    uint16_t *d_rows = m.at<uint16_t>(o_rows);
    uint8_t *d_rack = m.at<uint8_t>(o_rack);

    HIP_TRY(hipMemsetAsync(m.arena, 0, zeroed, st));
    HIP_TRY(hipMemcpyAsync(d_rack, rack_of, (size_t)B, hipMemcpyHostToDevice, st));
    if (P) HIP_TRY(hipMemcpyAsync(d_rows, rows, PW * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    int32_t launches = 0, ctl[FS_N] = {0};
    int max_n = 0, threads = 0;
    const size_t lds = (size_t)B * 16 + (size_t)((B + 31) / 32) * 4;
    if ((rc = fo_prelude(st, P, W, G, scope, d_rows, d_rack, d, reinterpret_cast<const void *>(k_fo_solve), lds, 48 * 1024, &launches, &max_n, &threads)))
        return rc;
    k_fo_solve<<<(unsigned)G, threads, lds, st>>>(B, W, scope, dry_run, d_rows, d_rack, d.lead, d.meta, d.cur, d.claim, d.cnt, d.off, d.start,
                                                 d.list, d_scen, d.ctl);
    HIP_TRY(hipGetLastError());
    ++launches;
    HIP_TRY(hipMemcpyAsync(ctl, d.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(scen, d_scen, (size_t)G * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctl[FS_ERR]) return fail(KAO_ERR_HIP, "kao_failover_order: a solve did not settle");
    if (!dry_run && P && ctl[FS_REORDERED]) {
        HIP_TRY(hipMemcpyAsync(rows, d_rows, PW * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *n_reordered = ctl[FS_REORDERED];
    if (stats) {
        for (int i = 0; i < 6; ++i) stats[i] = ctl[i];
        stats[6] = launches;
        stats[7] = max_n;
    }
    return KAO_OK;
}
