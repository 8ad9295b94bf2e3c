// kao_rccl.cpp -- the collectives of the multi-device paths (kao_rccl.h): the lazy librccl loader, the in-process loop-back table
// (test hook KAO_RCCL_LOOPBACK=1), the communicator cache, and the diagnostics kao_rccl_selftest / kao_rccl_loopback_counts.
#include <dlfcn.h>

#include <mutex>

#include "kao_rccl.h"
namespace {
// librccl.so is half a gigabyte of code objects; linking it would make every process that loads libkao.so (the CLI, a JVM)
// pay for registering them.  It is opened on the first multi-GPU exchange instead.
struct RcclLib : Rccl {
    void *h = nullptr;
    std::string why = "not found";   // text of the last dlopen / dlsym failure
    bool load() {
        if (h) return true;
        // RCCL must sit on the SAME HIP / HSA runtime instance this library runs on (a process may hold two: PyTorch wheels
        // bundle their own next to /opt/rocm's): look for librccl next to the libamdhip64 that serves our HIP calls first
        std::vector<std::string> names;
        Dl_info info;
        if (dladdr(reinterpret_cast<void *>(&hipGetDeviceCount), &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) { dir.resize(slash); names.push_back(dir + "/librccl.so.1"); names.push_back(dir + "/librccl.so"); }
        }
        names.push_back("librccl.so.1"); names.push_back("librccl.so"); names.push_back("/opt/rocm/lib/librccl.so.1");
        for (const std::string &name : names) {
            h = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (h) break;
            if (const char *e = dlerror()) why = e;   // dlerror() clears the message: read it once, here
        }
        if (!h) return false;
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(h, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(h, "ncclCommDestroy"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(h, "ncclGetErrorString"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(h, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(h, "ncclGroupEnd"));
        AllReduce = reinterpret_cast<decltype(AllReduce)>(dlsym(h, "ncclAllReduce"));
        Broadcast = reinterpret_cast<decltype(Broadcast)>(dlsym(h, "ncclBroadcast"));
        if (CommInitAll && CommDestroy && GetErrorString && GroupStart && GroupEnd && AllReduce && Broadcast) return true;
        if (const char *e = dlerror()) why = e; else why = "missing symbol";
        dlclose(h); h = nullptr;
        return false;
    }
} g_rccl;

// ---- loop-back collectives (test hook KAO_RCCL_LOOPBACK=1) ----------------------------------------------------------------
// The same function table filled with an in-process implementation: "ranks" are entries of the device list -- which may name
// one device several times -- and the two collectives kao_solve_multi uses move the data with plain copies when the group
// closes.  It exists so that the REAL control flow of the elite exchange (grouped ncclAllReduce(ncclUint64, ncclMin) on the
// resident key buffers, then one grouped ncclBroadcast per topic from the winner's rank) runs with several communicators on a
// box that has one GPU (the grouped sequence had never executed with more than one rank).  Never used unless the
// environment asks for it; results are those RCCL would deliver.
struct LoopComm { int rank, nranks, device; };
struct LoopOp { int kind; const void *send; void *recv; size_t count; int dtype, root; LoopComm *comm; hipStream_t st; int op; };
thread_local std::vector<LoopOp> t_loop_ops;
thread_local int t_loop_depth = 0;
uint64_t g_loop_allreduces = 0, g_loop_broadcasts = 0;   // collectives completed (test hook kao_rccl_loopback_counts)
size_t loop_elem(int dtype) { return dtype == ncclUint64 || dtype == ncclInt64 || dtype == ncclDouble ? 8 : (dtype == ncclUint8 || dtype == ncclInt8 ? 1 : 4); }
ncclResult_t loop_run() {
    std::vector<LoopOp> ops;
    ops.swap(t_loop_ops);
    if (ops.empty()) return ncclSuccess;
    const int n = ops[0].comm->nranks;
    if ((int)ops.size() != n) return ncclInvalidUsage;            // every rank of the communicator must take part
    std::vector<const LoopOp *> by_rank((size_t)n, nullptr);
    for (const LoopOp &o : ops) {
        if (o.kind != ops[0].kind || o.count != ops[0].count || o.dtype != ops[0].dtype || o.root != ops[0].root || o.op != ops[0].op || o.comm->nranks != n) return ncclInvalidUsage;
        if (o.comm->rank < 0 || o.comm->rank >= n || by_rank[(size_t)o.comm->rank]) return ncclInvalidUsage;
        by_rank[(size_t)o.comm->rank] = &o;
    }
    const size_t bytes = ops[0].count * loop_elem(ops[0].dtype);
    for (const LoopOp &o : ops)   // a collective is ordered behind the work already enqueued on each rank's stream
        if (hipSetDevice(o.comm->device) != hipSuccess || hipStreamSynchronize(o.st) != hipSuccess) return ncclUnhandledCudaError;
    if (ops[0].kind == 0 && ops[0].dtype == ncclDouble) {   // f64 sum / min (KAO-LP's shards): added in RANK order, every rank gets the same bits
        std::vector<double> acc(ops[0].count), tmp(ops[0].count);
        for (int r = 0; r < n; ++r) {
            const LoopOp &o = *by_rank[(size_t)r];
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(r ? tmp.data() : acc.data(), o.send, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
            if (r) for (size_t i = 0; i < acc.size(); ++i) acc[i] = ops[0].op == (int)ncclMin ? std::min(acc[i], tmp[i]) : acc[i] + tmp[i];
        }
        for (const LoopOp &o : ops)
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(o.recv, acc.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
        ++g_loop_allreduces;
    } else if (ops[0].kind == 0) {   // all-reduce: uint64 / min (the elite exchange)
        if (ops[0].dtype != ncclUint64) return ncclInvalidArgument;
        std::vector<uint64_t> acc(ops[0].count, ~0ull), tmp(ops[0].count);
        for (const LoopOp &o : ops) {
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(tmp.data(), o.send, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
            for (size_t i = 0; i < acc.size(); ++i) acc[i] = std::min(acc[i], tmp[i]);
        }
        for (const LoopOp &o : ops)
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(o.recv, acc.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
        ++g_loop_allreduces;
    } else {                  // broadcast from rank `root`
        if (ops[0].root < 0 || ops[0].root >= n) return ncclInvalidArgument;
        std::vector<unsigned char> buf(bytes);
        const LoopOp &r = *by_rank[(size_t)ops[0].root];
        if (hipSetDevice(r.comm->device) != hipSuccess || hipMemcpy(buf.data(), r.send, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
        for (const LoopOp &o : ops)
            if (hipSetDevice(o.comm->device) != hipSuccess || hipMemcpy(o.recv, buf.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
        ++g_loop_broadcasts;
    }
    return ncclSuccess;
}
ncclResult_t loop_CommInitAll(ncclComm_t *comms, int ndev, const int *devlist) {
    for (int i = 0; i < ndev; ++i) comms[i] = reinterpret_cast<ncclComm_t>(new LoopComm{i, ndev, devlist ? devlist[i] : i});
    return ncclSuccess;
}
ncclResult_t loop_CommDestroy(ncclComm_t c) { delete reinterpret_cast<LoopComm *>(c); return ncclSuccess; }
const char *loop_GetErrorString(ncclResult_t r) { return r == ncclSuccess ? "no error" : (r == ncclInvalidUsage ? "loop-back: invalid usage (a rank is missing from the group)" : "loop-back: error"); }
ncclResult_t loop_GroupStart() { ++t_loop_depth; return ncclSuccess; }
ncclResult_t loop_GroupEnd() { if (t_loop_depth <= 0) return ncclInvalidUsage; return --t_loop_depth == 0 ? loop_run() : ncclSuccess; }
ncclResult_t loop_AllReduce(const void *send, void *recv, size_t count, ncclDataType_t dt, ncclRedOp_t op, ncclComm_t c, hipStream_t st) {
    if (!((dt == ncclUint64 && op == ncclMin) || (dt == ncclDouble && (op == ncclMin || op == ncclSum)))) return ncclInvalidArgument;
    t_loop_ops.push_back(LoopOp{0, send, recv, count, (int)dt, 0, reinterpret_cast<LoopComm *>(c), st, (int)op});
    return t_loop_depth == 0 ? loop_run() : ncclSuccess;
}
ncclResult_t loop_Broadcast(const void *send, void *recv, size_t count, ncclDataType_t dt, int root, ncclComm_t c, hipStream_t st) {
    t_loop_ops.push_back(LoopOp{1, send, recv, count, (int)dt, root, reinterpret_cast<LoopComm *>(c), st, 0});
    return t_loop_depth == 0 ? loop_run() : ncclSuccess;
}
struct LoopTable : Rccl {
    LoopTable() {
        CommInitAll = &loop_CommInitAll; CommDestroy = &loop_CommDestroy; GetErrorString = &loop_GetErrorString;
        GroupStart = &loop_GroupStart; GroupEnd = &loop_GroupEnd; AllReduce = &loop_AllReduce; Broadcast = &loop_Broadcast;
    }
} g_loop;
struct CommSet { std::vector<int> devices; const Rccl *api; std::vector<ncclComm_t> comms; };
std::vector<CommSet> g_comms;   // communicators per (device list, function table) (creation costs ~100 ms with RCCL; kept until kao_shutdown)
std::mutex g_comm_mu;
}  // namespace

int kao::comms_for(const std::vector<int> &devices, std::vector<ncclComm_t> &out, const Rccl **api_out) {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    const bool loop = loopback_wanted();
    const Rccl *api = loop ? static_cast<const Rccl *>(&g_loop) : &g_rccl;
    *api_out = api;
    for (const CommSet &c : g_comms) if (c.devices == devices && c.api == api) { out = c.comms; return KAO_OK; }
    if (!loop && !g_rccl.load()) return fail(KAO_ERR_HIP, std::string("librccl.so not available: ") + g_rccl.why);
    for (int d : devices) {  // RCCL expects every device's primary context to exist already
        if (hipSetDevice(d) != hipSuccess || hipFree(nullptr) != hipSuccess) return fail(KAO_ERR_HIP, "cannot initialise device " + std::to_string(d));
        void *probe = nullptr;
        if (hipMalloc(&probe, 256) == hipSuccess) (void)hipFree(probe);
    }
    if (cur_device() >= 0) (void)hipSetDevice(cur_device());
    CommSet c; c.devices = devices; c.api = api; c.comms.resize(devices.size());
    const ncclResult_t r = api->CommInitAll(c.comms.data(), (int)devices.size(), devices.data());
    if (r != ncclSuccess) return fail(KAO_ERR_HIP, std::string("ncclCommInitAll: ") + api->GetErrorString(r));
    g_comms.push_back(c);
    out = c.comms;
    return KAO_OK;
}

extern "C" {
void kao_multi_shutdown_comms(void) {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    for (CommSet &c : g_comms) for (ncclComm_t cm : c.comms) (void)c.api->CommDestroy(cm);
    g_comms.clear();
}

// Diagnostic: the collectives kao_solve_multi uses, on small resident buffers of the listed (distinct) devices -- rank r holds
// keys {100 - r, 7 + r, ~0, r}; after ncclAllReduce(ncclUint64, ncclMin) every rank must hold {101 - n, 7, ~0, 0}, and after
// ncclBroadcast from the last rank every rank holds that rank's 64-byte pattern.  0 = ok.
int kao_rccl_selftest(const int32_t *devices, int32_t n_dev) {
    if (!devices || n_dev < 1 || n_dev > kMaxDevices) return fail(KAO_ERR_INVALID, "bad device list");
    std::vector<int> devs(devices, devices + n_dev);
    std::vector<ncclComm_t> comms;
    const Rccl *api = nullptr;
    int rc = comms_for(devs, comms, &api);
    if (rc) return rc;
    const Rccl &cc = *api;   // RCCL, or the loop-back table (KAO_RCCL_LOOPBACK=1: the list may then repeat a device)
    std::vector<unsigned long long *> keys((size_t)n_dev, nullptr), out((size_t)n_dev, nullptr);
    std::vector<unsigned char *> pat((size_t)n_dev, nullptr);
    std::vector<hipStream_t> st((size_t)n_dev, nullptr);
    bool ok = true;
    for (int d = 0; d < n_dev && ok; ++d) {
        ok = hipSetDevice(devs[(size_t)d]) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&keys[(size_t)d]), 32) == hipSuccess &&
             hipMalloc(reinterpret_cast<void **>(&out[(size_t)d]), 32) == hipSuccess && hipMalloc(reinterpret_cast<void **>(&pat[(size_t)d]), 64) == hipSuccess &&
             hipStreamCreateWithFlags(&st[(size_t)d], hipStreamNonBlocking) == hipSuccess;
        const unsigned long long h[4] = {100ull - (unsigned)d, 7ull + (unsigned)d, ~0ull, (unsigned long long)d};
        unsigned char p[64];
        for (int i = 0; i < 64; ++i) p[i] = (unsigned char)(d * 64 + i);
        ok = ok && hipMemcpy(keys[(size_t)d], h, 32, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(pat[(size_t)d], p, 64, hipMemcpyHostToDevice) == hipSuccess;
    }
    ncclResult_t nr = ok ? cc.GroupStart() : ncclSystemError;
    for (int d = 0; d < n_dev && nr == ncclSuccess; ++d) nr = cc.AllReduce(keys[(size_t)d], out[(size_t)d], 4, ncclUint64, ncclMin, comms[(size_t)d], st[(size_t)d]);
    if (nr == ncclSuccess) nr = cc.GroupEnd();
    if (nr == ncclSuccess) nr = cc.GroupStart();
    for (int d = 0; d < n_dev && nr == ncclSuccess; ++d) nr = cc.Broadcast(pat[(size_t)d], pat[(size_t)d], 64, ncclUint8, n_dev - 1, comms[(size_t)d], st[(size_t)d]);
    if (nr == ncclSuccess) nr = cc.GroupEnd();
    ok = ok && nr == ncclSuccess;
    for (int d = 0; d < n_dev && ok; ++d) {
        unsigned long long h[4]; unsigned char p[64];
        ok = hipSetDevice(devs[(size_t)d]) == hipSuccess && hipStreamSynchronize(st[(size_t)d]) == hipSuccess &&
             hipMemcpy(h, out[(size_t)d], 32, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(p, pat[(size_t)d], 64, hipMemcpyDeviceToHost) == hipSuccess;
        ok = ok && h[0] == 101ull - (unsigned)n_dev && h[1] == 7ull && h[2] == ~0ull && h[3] == 0ull;
        for (int i = 0; i < 64 && ok; ++i) ok = p[i] == (unsigned char)((n_dev - 1) * 64 + i);
    }
    for (int d = 0; d < n_dev; ++d) {
        (void)hipSetDevice(devs[(size_t)d]);
        (void)hipFree(keys[(size_t)d]); (void)hipFree(out[(size_t)d]); (void)hipFree(pat[(size_t)d]);
        if (st[(size_t)d]) (void)hipStreamDestroy(st[(size_t)d]);
    }
    if (cur_device() >= 0) (void)hipSetDevice(cur_device());
    if (!ok) return fail(KAO_ERR_HIP, nr != ncclSuccess ? std::string("RCCL: ") + cc.GetErrorString(nr) : std::string("RCCL self-test: wrong result"));
    return KAO_OK;
}

int kao_rccl_loopback_counts(uint64_t out[2]) {
    if (!out) return fail(KAO_ERR_INVALID, "null out");
    out[0] = g_loop_allreduces; out[1] = g_loop_broadcasts;
    return KAO_OK;
}
}  // extern "C"
