// tron_codes_io.hpp — how a kernel brings observation-code boards in and sends them out 16 bytes at a time, whatever a
// board's base address is (tron_playout.hip, tron_territory.hip): 16-byte aligned chunks put together with v_alignbyte;
// a chunk that sticks out of the caller's buffer is read byte by byte inside it, so no read ever leaves the buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tron {

// The 16 bytes at offset `at` (16-byte aligned as an address) of base[0, total); bytes outside the buffer read as 0 and are
// not loaded.
__device__ __forceinline__ uint4 chunk16(const int8_t *__restrict__ base, int64_t total, int64_t at)
{
    if (at >= 0 && at + 16 <= total) return *reinterpret_cast<const uint4 *>(base + at);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (at + i >= 0 && at + i < total) w[i >> 2] |= (uint32_t)(uint8_t)base[at + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// The 16 bytes at offset f of base[0, total) from the two aligned chunks that hold them.
__device__ __forceinline__ void load16(const int8_t *__restrict__ base, int64_t total, int64_t f, uint32_t out[4])
{
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(base + f) & 15u);
    const uint4 c0 = chunk16(base, total, f - mis), c1 = mis ? chunk16(base, total, f - mis + 16) : make_uint4(0u, 0u, 0u, 0u);
    uint32_t t[9] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, 0u};
    if (mis & 8u) {
#pragma unroll
        for (int j = 0; j < 7; ++j) t[j] = t[j + 2];
    }
    if (mis & 4u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = t[j + 1];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = __builtin_amdgcn_alignbyte(t[j + 1], t[j], mis & 3u);
}
// The first nvalid of 16 bytes to p: one 16-byte store where p allows it, dwords where it allows those, else bytes.
__device__ __forceinline__ void store16(int8_t *p, int nvalid, const uint32_t x[4])
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (nvalid == 16 && (a & 15u) == 0u) {
        *reinterpret_cast<uint4 *>(p) = make_uint4(x[0], x[1], x[2], x[3]);
        return;
    }
    const bool dwords = (a & 3u) == 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (dwords && 4 * j + 4 <= nvalid) {
            reinterpret_cast<uint32_t *>(p)[j] = x[j];
        } else {
#pragma unroll
            for (int i = 4 * j; i < 4 * j + 4; ++i)
                if (i < nvalid) p[i] = (int8_t)(x[j] >> (8 * (i & 3)));
        }
    }
}

}  // namespace tron
