// kao_host.h -- host-side internals shared by the translation units behind the C ABI (include/kao.h):
//   kao_model.cpp    the model on the host: validation, bands, dense -> rack-major index, infeasibility proofs, the closed-form
//                    upper bound (kao_upper_bound)
//   kao_runtime.cpp  device selection, error text, kao_init / kao_shutdown, the pools of parked arenas and streams
//   kao_evalplan.cpp K-eval plans, kao_evaluate(_batch), the canonical tie-break (kao_canonicalize)
//   kao_session.cpp  sessions: the plan of a batch of topics on one device (options, pools, launch groups, arena layout), its
//                    upload, the K-search / K-eval step, the read-back
//   kao_session_bound.cpp  K-bound on a session: launches, search prices, bounds, dual state; kao_dual_bound
//   kao_lp_api.cpp   the one-shot KAO-LP entry points (kao_lp_bound / _round / _round_host / _trace)
//   kao_solve.cpp    the solve loops on top of sessions: kao_solve, kao_solve_multi (several devices in lockstep), and the readers of the
//                    last solve's counters (kao_last_solve_timing / _lp / _profile)
//   kao_rccl.cpp     the collectives of the multi-device paths (kao_rccl.h): the lazy librccl loader, the loop-back table, communicators
//   kao_lp_fan.cpp   ONE LP sharded over several devices (lp_open_fan, kao_lp_sharded_test)
//   kao_capped.cpp   kao_solve_capped: Lagrangian prices over kao_solve / kao_solve_multi, through the C ABI only
//   kao_pairs.cpp    compound edges of leader-balanced pairs for KAO-CX;  kao_round.cpp  KAO-LP's primal side: the iterate rounded to an assignment
//   kao_waves.hip    kao_plan_waves(_sized): a reassignment plan split into waves
//   kao_leaders.hip, kao_leaders_cluster.hip, kao_wleaders.hip, kao_failover.hip, kao_wfailover.hip, kao_disk.hip, kao_logdirs.hip  the one-shot planners of
//                    leaders, follower orders and replica moves by disk usage, between brokers and between the log dirs of one (kernels and entry point in one file each; device code they share: kao_plan_dev.h, the
//                    failover scenario passes: kao_failover_dev.h; host code they share: "one-shot planner calls" below)
// Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kao.h"
#include "kao_internal.h"

namespace kao {

// ---- runtime (kao_runtime.cpp) ----
int fail(int code, const std::string &msg);   // records the text kao_last_error returns; returns `code`
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::kao::fail(KAO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
double now_s();
int cur_device();                 // the calling thread's device: t_device when set, else the process default (kao_init)
constexpr int kMaxDevices = 64;   // device ordinals the per-device tables cover
int num_cu(int device);
int require_init();               // kao_init on first use, then hipSetDevice(cur_device())
bool is_init();
extern thread_local int t_device; // per-thread override: kao_solve_multi drives several devices from one process (assigned through DeviceScope only)
// The calling thread on another device for the scope's life: `to` sets the override and makes the device current (`rc`: how the last
// switch went), and moves an open scope on to the next device of a list; the destructor puts the previous override back and makes
// cur_device() current again.  Objects that close device resources in their destructors are declared AFTER the scope they live under.
struct DeviceScope {
    const int saved = t_device;
    int rc = KAO_OK;
    DeviceScope() = default;
    explicit DeviceScope(int device) { to(device); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    int to(int device);
    ~DeviceScope();
};
// The counters of this thread's last solve, under the names solver.py gives them; kao_last_solve_timing / _lp / _profile (kao_solve.cpp)
// alone know the array layout of include/kao.h.  Times are seconds from the solve's entry; counts are kept as doubles, as they are returned.
struct SolveTiming {
    double session_ready, time_to_best, results_read_back, returned, launches, delta_candidates, bound_launches, elite_exchanges,
           bound_iters, cx_calls, cx_gains, search_iters, generations, cx_further_starts, lp_solves, lp_iters;
};
struct SolveLp { double solves, iterations, rounded, adopted, fractional_partitions; };   // KAO-LP in the last kao_solve
struct SolveProfile {   // K-search as the last profiled kao_solve ran it
    double ms_search, ms_eval, search_launches, restarts, search_bytes_algo, delta_candidates, lds_bytes_search, blocks_search;
};
struct SolveCounters { SolveTiming timing; SolveLp lp; SolveProfile profile; };
extern thread_local SolveCounters g_last;   // (kao_solve.cpp)
// The KAO_* environment hooks (tests, measurements, diagnostics): an unset or empty variable gives `dflt`.
// Every read of the environment in csrc/ goes through these; the kernel files read none.
inline const char *env_str(const char *name) { const char *e = std::getenv(name); return e && *e ? e : nullptr; }
inline int64_t env_int(const char *name, int64_t dflt) { const char *e = env_str(name); return e ? (int64_t)std::atoll(e) : dflt; }
inline double env_real(const char *name, double dflt) { const char *e = env_str(name); return e ? std::atof(e) : dflt; }
// hipMalloc / hipFree cost 0.1-1 ms each, a stream ~1 ms: finished sessions park their arenas and streams here for the next one
int arena_get(size_t bytes, void **out, size_t *cap);   // a parked arena of the current device that fits, else hipMalloc
void arena_put(void *p, size_t bytes, int device);
int stream_get(hipStream_t *out);
void stream_put(hipStream_t st, int device);
void arena_drop_all();
inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
// LDS / register form of a replica: internal (rack-major) index | rack << 16, m = the largest rack
inline uint32_t replica_word(uint16_t x, int m) { return x == KAO_NONE ? kNoneW : ((uint32_t)x | ((uint32_t)(x / m) << 16)); }

// ---- one-shot planner calls (kao_runtime.cpp): what the leader and failover planners share on the host ----
// The device memory and the stream of one call, handed back to the runtime's pools on every return path.
struct CallBufs {
    void *arena = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    CallBufs() = default;
    CallBufs(const CallBufs &) = delete;
    CallBufs &operator=(const CallBufs &) = delete;
    int open(size_t bytes);   // arena_get, then stream_get
    template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(static_cast<unsigned char *>(arena) + off); }
    ~CallBufs();              // synchronises the stream
};
// The layout of one call's arena: take<T>(count) is the offset of the next buffer, each one aligned to 256 bytes; end() is where the
// next one would start (the total, or the end of a prefix that one memset or copy covers).
struct Carve {
    size_t next = 0;
    template <class T> size_t take(size_t count) { const size_t o = next; next += align_up(count * sizeof(T)); return o; }
    size_t end() const { return next; }
};
inline unsigned grid_for(int64_t n, int threads) { return (unsigned)((std::max<int64_t>(n, 1) + threads - 1) / threads); }
// Argument checks; `fn` is the text in front of every message ("kao_...: ").  check_dims: width, brokers, racks (of the calls that
// have them), partitions, in that order.  check_row: slot 0 holds a broker, no broker after an empty slot, every index below
// n_brokers, no broker twice; check_rows: every row.
int check_dims(const std::string &fn, int32_t B, int32_t P, int32_t W, int32_t R = 1);
int check_slot_cap(const std::string &fn, int32_t P, int32_t W);   // 4,000,000 replica slots
int check_row(const std::string &fn, int32_t B, int32_t W, int64_t p, const uint16_t *row);
int check_rows(const std::string &fn, int32_t B, int32_t P, int32_t W, const uint16_t *rows);
int check_weight_sum(const std::string &fn, int32_t P, const uint64_t *weight);   // below 2^62: every load of the kernels stays below 2^63
// The relaxation rounds of one phase of successive shortest paths (kao_plan_dev.h: flow keys): launch(r, flag) enqueues round r,
// whose kernel sets *flag when it changed a key.  kSettleBatch rounds are enqueued between two reads of the flags (the seed kernel
// cleared them for the first batch); `rounds` counts up to and including the first round that changed nothing.  N = the nodes: keys
// settle within N rounds.
constexpr int kSettleBatch = 8;
template <class Launch>
int settle_rounds(const char *fn, hipStream_t st, int N, int32_t *d_flags, int32_t &rounds, int32_t &launches, Launch launch) {
    int32_t flags[kSettleBatch];
    for (int r = 0, settled = 0; !settled;) {
        if (r > N + kSettleBatch) return fail(KAO_ERR_HIP, std::string(fn) + "relaxation did not settle");
        if (r) { HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof flags, st)); }
        for (int i = 0; i < kSettleBatch; ++i, ++r) launch(r, d_flags + i);
        launches += kSettleBatch;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < kSettleBatch && !settled; ++i) {   // the first round that changed nothing ends the phase's rounds
            ++rounds;
            settled = flags[i] == 0;
        }
    }
    return KAO_OK;
}

// ---- the model on the host (kao_model.cpp) ----
int validate(const kao_topic *t);
void derive_bounds(const kao_topic *t, int32_t o[8]);
// Host-side image of one topic in both index spaces.
struct PreparedTopic {
    TopicDev d{};
    std::vector<uint16_t> int_of;   // dense -> internal
    std::vector<uint16_t> ext_of;   // internal -> dense
    std::vector<int32_t> rack_size; // [R]
    std::vector<uint16_t> cur_int;  // [P*4] internal
    std::vector<uint8_t> rack_of;   // [B]
    std::vector<uint16_t> cur_dense;// [P*rf_cur]
    std::vector<uint32_t> bw_int, bw_dense;  // broker weights bw | bwl << 16 per internal / dense index (empty = none)
};
int prepare(const kao_topic *t, uint64_t seed, PreparedTopic &pt);
std::string infeasible_reason(const kao_topic *t);
int64_t upper_bound(const kao_topic *t);
int64_t upper_bound_w(const kao_topic *t);     // ... of a topic that may carry broker weights
uint64_t neighbours_in_range(uint32_t it0, uint32_t iters, int rf, int n_brokers, int n_partitions, int scan2_max = kScanTwoSlots);
int auto_period_log2(int P, int RF);
bool dual_supported(const kao_topic *t, bool session_bw = false);       // within K-bound's limits (session_bw: the session carves broker weights)

}  // namespace kao

using namespace kao;

struct kao_eval_plan {
    PreparedTopic pt;
    TopicDev *d_topic = nullptr;
    uint8_t *d_rackof = nullptr;
    uint16_t *d_curd = nullptr;
    int4 *d_map = nullptr;
    uint32_t *d_bwd = nullptr;      // broker weights (dense) when the topic has them
    int32_t *d_overflow = nullptr;  // set by K-eval when a candidate overflows a 16-bit per-broker counter (P*RF > 65535 only)
    int64_t map_n = -1;
    int map_blocks = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    int cands_per_block = 32;
    bool cur_in_lds = true;
    bool coop = false;            // the last batch ran one candidate per workgroup (k_eval<NE, true>)
    int device = 0;
};

struct kao_session {
    int device = 0;              // HIP device this session lives on
    int n_topics = 0;
    kao_opts opts{};
    std::vector<PreparedTopic> pts;
    std::vector<kao_topic> topics;  // shallow copies (pointers not retained for device work)
    std::vector<int64_t> ub;
    std::vector<char> topic_global;  // per topic: runs with its assignment in global memory
    std::vector<char> topic_curg;    // per topic: working assignment in LDS, current assignment from global memory (k_search_curg)
    std::vector<char> topic_infeasible;  // per topic: proven infeasible by counting (kao_check_infeasible)
    std::vector<char> dual_ok;           // per topic: within K-bound's limits
    std::vector<int64_t> h_dual_target;  // staging for kao_session_bound_step
    std::vector<int32_t> h_dual_ids;
    bool multi_off = false;              // k_bound_multi gave up once in this session (kao_session_bounds): the step kernels from then on
    std::vector<int2> h_wide_map;        // sliced K-bound: {topic, slice} per workgroup (staging, like h_dual_ids)
    uint64_t wide_ctl_i32 = 0, wide_map_i32 = 0;   // int32 offsets of the control blocks / the map inside d_dual
    std::vector<int32_t> dual_flags, dual_iters;
    int total_restarts = 0;
    // Topics are bucketed by LDS footprint into launch groups (a 3000-partition topic must not impose its LDS carve
    // and its 2 waves per workgroup on 200 small topics); one K-search + one K-eval launch per group per step.
    struct LaunchGroup {
        int maxP = 0, maxBx = 0, maxB = 0, maxR = 0;
        bool wide = false;   // some topic of the group has 512 replica slots or more (several tournament slots per lane)
        int waves = kWaves;  // restarts per K-search workgroup: 4, 2 or 1 -- the largest whose LDS carve fits 160 KiB
        int nw = kRFP;       // replica words per partition of the group's topics: 4 or 8 (template instantiation)
        int rf_uniform = -1; // the RF all topics of the group share (0: mixed; -1: no topic yet)
        int w_abs_max = 0;   // the largest |w00..w11| over the group's topics (search_small_cost)
        bool band_tabs = true;   // every topic's replica and leader band fits a band-row table (search_band_tabs): the small-cost form may run
        bool rf3 = true;     // every topic has RF 3 and at most 3 current replicas per partition: K-search may run its RF-3 instantiation
        bool global_a = false;   // topic too large for LDS: assignment + current words stay in global memory
        bool cur_global = false; // (round 5) only the current-assignment words stay in global memory / L2, the working words are in LDS (~4,900 .. 9,800 partitions)
        int team = 0;            // > 0 (global_a only): every restart is searched by a TEAM of that many wavefronts (k_team), one workgroup per restart
        bool cur_in_lds = true;  // K-eval stages the current assignment in LDS (false: reads it from global)
        bool eval_coop = false;  // K-eval: one candidate per workgroup, wavefronts cooperating (few large candidates)
        int smap_off = 0, smap_n = 0, emap_off = 0, emap_n = 0;
        // K-search as ticketed chunks (plan_chunks): tickets of a launch (0 = one piece per entry, the launch as it always was), chunks
        // per entry, the group's first record in d_sched, the iterations per launch and the pricing the schedule was made for
        int chunk_tickets = 0, chunk_n = 0, sched_off = 0, chunk_iters = 0;
        bool chunk_priced = false;
    };
    std::vector<LaunchGroup> groups;
    int blocks_search = 0, blocks_eval = 0;
    // device memory: one read-only arena (instance tables, uploaded with ONE H2D copy) and one mutable
    // arena (restart states, snapshots, results); the pointers below are carved from them
    void *arena_ro = nullptr, *arena_rw = nullptr;
    size_t arena_ro_bytes = 0, arena_rw_bytes = 0;
    TopicDev *d_topics = nullptr;
    int2 *d_smap = nullptr;
    int4 *d_emap = nullptr;
    uint32_t *d_cur = nullptr;
    uint16_t *d_ext = nullptr;
    int32_t *d_rsz = nullptr;
    uint8_t *d_rackof = nullptr;
    uint16_t *d_curd = nullptr;
    unsigned char *d_state = nullptr;
    uint16_t *d_best = nullptr;
    int32_t *d_info = nullptr;
    int32_t *d_obj = nullptr;
    int32_t *d_viol = nullptr;
    // read-back block (contiguous): [keys u64[T]] [drift i32 (16 B)] [win_viol i32[8T]] [win_assign u16[sum P*RF]]
    unsigned char *d_readback = nullptr;
    size_t readback_bytes = 0, rb_viol_off = 0, rb_assign_off = 0;
    // K-bound: multipliers + directions per topic; targets and workgroup->topic ids (host-written before a launch);
    // read-back block [best_L i64[T]] [info i32[4T]]
    int32_t *d_dual = nullptr;
    // search prices, double buffered: K-bound launch n exports into half (n & 1) while K-search reads the half of the last
    // launch whose results the host has merged (price_read); topics K-bound never covered read zeros
    int32_t *d_price = nullptr;
    size_t price_half_i32 = 0;
    int price_read = 0;          // half K-search reads
    int price_write_last = -1;   // half the K-bound launch in flight (or the last finished one) writes
    bool priced = false;         // K-search launches carry prices
    bool any_bw = false;         // some topic carries broker weights (their LDS table is carved in every launch group)
    uint16_t *d_int = nullptr;   // dense -> internal broker index per topic
    uint32_t *d_bw = nullptr, *d_bwd = nullptr;   // broker weights per internal / dense index (topics with has_bw)
    long long *d_dual_target = nullptr;
    int32_t *d_dual_ids = nullptr;
    unsigned char *d_dual_rb = nullptr;
    size_t dual_rb_bytes = 0;
    uint64_t bound_launches = 0;
    bool dual_state_init = false;   // the K-bound state in HBM has been cleared (first launch or kao_session_set_dual_state)
    size_t dual_bytes = 0;
    hipStream_t stream_bound = nullptr;   // K-bound runs beside K-search on its own stream (it occupies one CU per topic)
    hipEvent_t ev_bound0 = nullptr, ev_bound1 = nullptr, ev_search = nullptr;
    bool bound_inflight = false;
    bool bound_no_wait = false;  // kao_solve's deterministic schedule: no event wait on the search stream before a K-bound launch
    int bound_iters_last = 0;
    double bound_ms_last = 0;
    unsigned long long *d_keys = nullptr;
    unsigned long long *d_keys_glob = nullptr;  // receive buffer of the cross-GPU min-allreduce (kao_solve_multi)
    int32_t *d_drift = nullptr;
    int32_t *d_win_viol = nullptr;
    uint16_t *d_win_assign = nullptr;
    std::vector<unsigned char> h_readback;
    hipStream_t stream = nullptr;
    uint32_t launch = 0;
    uint32_t gen = 0;            // generation of the population (kao_session_new_generation)
    bool reinit = false;         // the next step re-initialises every restart (first launch of a new generation)
    size_t best_bytes = 0;       // size of the snapshot pool d_best
    // profiling
    std::vector<hipEvent_t> ev;  // triples
    int ev_pending = 0;
    double ms_search = 0, ms_eval = 0;
    uint64_t eval_bytes_per_launch = 0;
    uint64_t delta_total = 0, search_bytes_total = 0;
    uint64_t search_rf3_launches = 0;   // K-search launches that ran the RF-3 instantiation (kao_stats)
    uint64_t search_small_launches = 0; // of those, the launches that ran its small-cost form (kao_session_small_launches)
    bool small_on = true;               // KAO_SEARCH_SMALL (read when the session is created; 0 = never the small-cost form)
    // K-search as ticketed chunks (kao.h: kao_session_chunked_launches).  The buffers exist only in sessions with a group that chunks.
    int chunks_forced = 0;               // KAO_SEARCH_CHUNKS (read when the session is created): 0 automatic, 1 never, N >= 2 forced
    bool can_chunk = false;              // some launch group runs chunked
    int4 *d_sched = nullptr;             // the groups' schedules (read-only arena)
    uint32_t *d_chunk_ctl = nullptr;     // [0] the ticket counter (zero between launches: the holder of the last ticket resets it)
    uint32_t *d_chunk_progress = nullptr;// one word per block-map entry: launch serial * 256 + chunks done
    uint32_t *d_chunk_rng = nullptr;     // 64 generator words per restart, handed from chunk to chunk
    uint32_t chunk_serial = 0;           // serial of the last chunked launch (the progress words carry it: nothing is cleared per launch)
    uint64_t search_chunked_launches = 0;
    int32_t *h_chunk_err = nullptr;      // chunking sessions: pinned read-back of the error word behind the drift counter.  Once set it stays
                                         // set (nothing clears the device word): every later synchronising call of the session fails
};

namespace kao {
// K-bound's dual values are fixed point (kDualScale); a bound on the integer objective is their floor -- unless the launch flagged the
// value unusable (flag 4) or no iteration has run
constexpr int64_t kDualNone = 0x7F7F7F7F7F7F7F7Fll;   // best dual value "none yet" (the state is cleared with bytes of 0x7F)
inline int64_t dual_floor(int64_t best_dual) { return best_dual >= 0 ? best_dual / kDualScale : -((-best_dual + kDualScale - 1) / kDualScale); }
inline int64_t dual_bound_value(int32_t flags, int32_t iters, int64_t best_dual) { return (flags & 4) || iters == 0 ? INT64_MAX : dual_floor(best_dual); }
struct SessionDeleter { void operator()(kao_session *s) const { kao_session_destroy(s); } };
using SessionPtr = std::unique_ptr<kao_session, SessionDeleter>;   // a session on its way out of kao_session_create, or a throw-away one
int bound_only_session(const kao_topic *t, SessionPtr &out);   // one topic, no search: K-bound alone (kao_session_bound.cpp); fails outside K-bound's limits
// the topic's winning assignment (dense [P*RF]) as of the last finished launch
int session_topic_best(kao_session *s, int i, uint16_t *out);
// every restart's best feasible objective (-1 = none yet) / one restart's best snapshot, as of the last finished launch
int session_restart_objs(kao_session *s, int i, std::vector<int32_t> &objs);
int session_restart_best(kao_session *s, int i, int restart, uint16_t *out);
// an assignment found outside K-search (KAO-CX, another GPU) becomes the topic's incumbent and elite
int session_adopt_external(kao_session *s, int i, const uint16_t *assign, int64_t objective, uint64_t *key_out);
}  // namespace kao
