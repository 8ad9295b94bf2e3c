// kao_rccl.h -- what the host units that use collectives share (kao_rccl.cpp, kao_solve.cpp, kao_lp_fan.cpp): the function table both
// transports fill (librccl, opened on first use, and the in-process loop-back table) and the communicator cache.  The only place that
// includes <rccl/rccl.h>; not for the .hip units.
#pragma once
#include <rccl/rccl.h>  // types and prototypes only: librccl.so is loaded on first use (kao_rccl.cpp)

#include "kao_host.h"

namespace kao {
#pragma GCC visibility push(hidden)
struct Rccl {
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
};
inline bool loopback_wanted() { return env_int("KAO_RCCL_LOOPBACK", 0) != 0; }
// the communicators of a device list (created once, kept until kao_multi_shutdown_comms) and the table that serves them: RCCL, or the
// loop-back table when KAO_RCCL_LOOPBACK=1 (the list may then name a device several times)
int comms_for(const std::vector<int> &devices, std::vector<ncclComm_t> &out, const Rccl **api_out);
#pragma GCC visibility pop
}  // namespace kao
