// kao_bytes_code.h -- the monotone 16-bit code of a 64-bit quantity that the wave planner (kao_waves.hip), the traffic-weighted
// planners (kao_wleaders.hip, kao_wfailover.hip) and the disk-usage and log-dir balances (kao_disk.hip, kao_logdirs.hip) put into their
// priority keys.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// monotone 16-bit code of a byte count: 0 -> 0; otherwise (bit length e, 1..64) << 9 | the 9 bits below the leading one
// (truncated), at most 64 << 9 | 511 = 33,279.  A logarithmic scale with a 9-bit mantissa, integer-only.
__device__ inline uint32_t wave_bytes_code(uint64_t t) {
    if (t == 0) return 0;
    const int e = 64 - __clzll((long long)t);
    return (uint32_t)e << 9 | (uint32_t)((t << (64 - e)) >> 54 & 0x1FFu);
}
