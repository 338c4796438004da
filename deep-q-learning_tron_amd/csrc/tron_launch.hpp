// tron_launch.hpp — what every launcher of a big-LDS kernel does on the host before it launches, stated once.  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tron_hip.h"

namespace tron {

// the current device's ordinal into dev; no device is TRON_ERR_NO_DEVICE, with HIP's sticky error cleared
inline int current_device(int &dev)
{
    if (hipGetDevice(&dev) == hipSuccess) return TRON_OK;
    (void)hipGetLastError();
    return TRON_ERR_NO_DEVICE;
}

// More than 64 KB of dynamic LDS needs an opt-in per kernel, and the attribute is set on the current device only: remember,
// per kernel, which devices it was prepared on (one bit per device ordinal) instead of a per-process flag.  A refusal is not
// reported here: the launch that follows fails and says so.  Not thread-safe, like the launchers that call it.
template <auto Kernel>
void allow_lds(int dev, int bytes)
{
    static uint64_t prepared = 0;
    const uint64_t bit = 1ull << (dev & 63);
    if (prepared & bit) return;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        (void)hipGetLastError();
    prepared |= bit;
}

// compute units of device dev, asked once per device; 256 (an MI355X) where the query fails
inline int device_cus(int dev)
{
    static int cus[64];
    static uint64_t known = 0;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(known & bit)) {
        hipDeviceProp_t prop;
        cus[dev & 63] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : 256;
        (void)hipGetLastError();
        known |= bit;
    }
    return cus[dev & 63];
}

}  // namespace tron
