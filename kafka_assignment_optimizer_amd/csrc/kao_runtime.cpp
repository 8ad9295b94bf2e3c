// kao_runtime.cpp -- the runtime every other host file of libkao.so stands on (see kao_host.h): device selection and DeviceScope,
// the error text, kao_init / kao_shutdown, and the pools that park device arenas and streams between sessions.
#include <chrono>
#include <cstdio>
#include <mutex>

#include "kao_host.h"

namespace kao {

thread_local int t_device = -1;

namespace {
thread_local std::string g_err;
int g_device = -1;           // the process default (kao_init)
bool g_init = false;
int g_num_cu_of[kMaxDevices] = {0};
}  // namespace

int cur_device() { return t_device >= 0 ? t_device : g_device; }
int DeviceScope::to(int device) {
    t_device = device;
    return rc = hipSetDevice(device) == hipSuccess ? KAO_OK : fail(KAO_ERR_NO_DEVICE, "hipSetDevice");
}
DeviceScope::~DeviceScope() { t_device = saved; if (cur_device() >= 0) (void)hipSetDevice(cur_device()); }
int num_cu(int device) {
    if (device < 0 || device >= kMaxDevices) return 256;
    if (!g_num_cu_of[device]) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0) v = 256;
        g_num_cu_of[device] = v;
    }
    return g_num_cu_of[device];
}

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

double now_s() {
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

bool is_init() { return g_init; }
int require_init() {
    if (!g_init) {
        int rc = kao_init(g_device < 0 ? 0 : g_device);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(cur_device()));
    return KAO_OK;
}

// the same three for the device translation units (kao_internal.h), which do not see kao_host.h
int api_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
int api_require_init() { return require_init(); }
double api_now_s() { return now_s(); }

namespace {
// hipMalloc / hipFree cost 0.1-1 ms each; a finished session parks its arenas here for the next one
struct Parked { void *p; size_t bytes; int device; };
std::vector<Parked> g_parked;
constexpr size_t kParkMax = 4;
std::vector<std::pair<hipStream_t, int>> g_streams;  // parked streams with their device (create/destroy cost ~1 ms)
std::mutex g_cache_mu;  // guards g_parked / g_streams (sessions may be created from several host threads)
}  // namespace

int arena_get(size_t bytes, void **out, size_t *cap) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    const int dev = cur_device();
    size_t best = g_parked.size();
    for (size_t i = 0; i < g_parked.size(); ++i)
        if (g_parked[i].device == dev && g_parked[i].bytes >= bytes && g_parked[i].bytes <= 4 * bytes + (1u << 20) &&
            (best == g_parked.size() || g_parked[i].bytes < g_parked[best].bytes)) best = i;
    if (best < g_parked.size()) {
        *out = g_parked[best].p; *cap = g_parked[best].bytes;
        g_parked.erase(g_parked.begin() + (long)best);
        return KAO_OK;
    }
    const size_t want = ((bytes + (1u << 16)) + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc(out, want));
    *cap = want;
    return KAO_OK;
}
void arena_put(void *p, size_t bytes, int device) {
    if (!p) return;
    std::lock_guard<std::mutex> lock(g_cache_mu);
    (void)hipSetDevice(device);
    if (g_parked.size() >= kParkMax) {
        size_t small = 0;
        for (size_t i = 1; i < g_parked.size(); ++i) if (g_parked[i].bytes < g_parked[small].bytes) small = i;
        if (g_parked[small].bytes >= bytes) { (void)hipFree(p); return; }
        (void)hipSetDevice(g_parked[small].device);
        (void)hipFree(g_parked[small].p);
        (void)hipSetDevice(device);
        g_parked.erase(g_parked.begin() + (long)small);
    }
    g_parked.push_back({p, bytes, device});
}
int stream_get(hipStream_t *out) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    const int dev = cur_device();
    for (size_t i = 0; i < g_streams.size(); ++i)
        if (g_streams[i].second == dev) { *out = g_streams[i].first; g_streams.erase(g_streams.begin() + (long)i); return KAO_OK; }
    HIP_TRY(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return KAO_OK;
}
void stream_put(hipStream_t st, int device) {
    if (!st) return;
    std::lock_guard<std::mutex> lock(g_cache_mu);
    if (g_streams.size() < 16) g_streams.push_back({st, device}); else { (void)hipSetDevice(device); (void)hipStreamDestroy(st); }
}
void arena_drop_all() {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    for (auto &a : g_parked) { (void)hipSetDevice(a.device); (void)hipFree(a.p); }
    g_parked.clear();
    for (auto &st : g_streams) { (void)hipSetDevice(st.second); (void)hipStreamDestroy(st.first); }
    g_streams.clear();
    if (g_device >= 0) (void)hipSetDevice(g_device);
}

// ---- one-shot planner calls ----
int CallBufs::open(size_t bytes) {
    int rc = arena_get(bytes, &arena, &cap);
    return rc ? rc : stream_get(&stream);
}
CallBufs::~CallBufs() {
    if (stream) { (void)hipStreamSynchronize(stream); stream_put(stream, cur_device()); }
    if (arena) arena_put(arena, cap, cur_device());
}

int check_dims(const std::string &fn, int32_t B, int32_t P, int32_t W, int32_t R) {
    if (W < 1 || W > KAO_MAX_RF) return fail(KAO_ERR_INVALID, fn + "width outside 1.." + std::to_string(KAO_MAX_RF));
    if (B < 1 || B > 65534) return fail(KAO_ERR_INVALID, fn + "n_brokers outside 1..65534");
    if (R < 1 || R > KAO_MAX_RACKS) return fail(KAO_ERR_INVALID, fn + "n_racks outside 1.." + std::to_string(KAO_MAX_RACKS));
    if (P < 0) return fail(KAO_ERR_INVALID, fn + "n_partitions < 0");
    return KAO_OK;
}
int check_slot_cap(const std::string &fn, int32_t P, int32_t W) {
    return (int64_t)P * W > 4000000 ? fail(KAO_ERR_UNSUPPORTED, fn + "more than 4,000,000 replica slots") : KAO_OK;
}
int check_row(const std::string &fn, int32_t B, int32_t W, int64_t p, const uint16_t *row) {
    const auto bad = [&](const char *what) { return fail(KAO_ERR_INVALID, fn + "partition " + std::to_string(p) + ": " + what); };
    if (row[0] == KAO_NONE) return bad("slot 0 holds no broker");
    bool ended = false;
    for (int i = 0; i < W; ++i) {
        if (row[i] == KAO_NONE) { ended = true; continue; }
        if (ended) return bad("a broker after an empty slot");
        if (row[i] >= B) return bad("broker index >= n_brokers");
        for (int j = 0; j < i; ++j)
            if (row[j] == row[i]) return bad("broker repeated in a row");
    }
    return KAO_OK;
}
int check_rows(const std::string &fn, int32_t B, int32_t P, int32_t W, const uint16_t *rows) {
    int rc = KAO_OK;
    for (int64_t p = 0; p < P && !rc; ++p) rc = check_row(fn, B, W, p, rows + p * W);
    return rc;
}
int check_weight_sum(const std::string &fn, int32_t P, const uint64_t *weight) {
    uint64_t total = 0;
    for (int64_t p = 0; p < P; ++p)
        if (__builtin_add_overflow(total, weight[p], &total) || total >= (uint64_t(1) << 62))
            return fail(KAO_ERR_INVALID, fn + "partition " + std::to_string(p) + ": the weights sum to 2^62 or more");
    return KAO_OK;
}

}  // namespace kao

extern "C" {

int kao_version(void) { return KAO_VERSION; }

const char *kao_strerror(int code) {
    switch (code) {
        case KAO_OK: return "ok";
        case KAO_ERR_INVALID: return "invalid argument";
        case KAO_ERR_UNSUPPORTED: return "instance not supported by the gfx950 kernels";
        case KAO_ERR_NO_DEVICE: return "no usable HIP device (libkao has no CPU fallback)";
        case KAO_ERR_HIP: return "HIP runtime error";
        case KAO_ERR_NOMEM: return "out of memory";
        case KAO_ERR_NOT_INIT: return "kao_init not called";
        default: return "unknown error";
    }
}

const char *kao_last_error(void) { return g_err.c_str(); }

int kao_init(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(KAO_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(KAO_ERR_INVALID, "device ordinal out of range");
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(KAO_ERR_NO_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    (void)num_cu(device);
    g_device = device;
    g_init = true;
    return KAO_OK;
}

void kao_multi_shutdown_comms(void);

void kao_shutdown(void) {
    kao_multi_shutdown_comms();
    if (g_init) arena_drop_all();
    g_init = false;
}

int kao_device_name(char *buf, int len) {
    int rc = require_init();
    if (rc) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cur_device()));
    std::snprintf(buf, (size_t)len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return KAO_OK;
}

}  // extern "C"
