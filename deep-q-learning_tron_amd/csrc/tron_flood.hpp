// tron_flood.hpp — what the level-synchronous bitboard floods share (tron_minimax.hip's voronoi(),
// tron_territory.hip).  One lane per board ROW, the row a bit mask (bit c = column c): left / right are shifts within the
// mask, up / down one whole-wave DPP shift each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tron {

// whole-wave shifts by one lane on the DPP path (no LDS crossbar round trip): wave_shr:1 hands lane
// r the value of lane r-1, wave_shl:1 that of lane r+1; the lane with no source keeps `old` = 0
__device__ __forceinline__ uint32_t dpp_from_above(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t dpp_from_below(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xF, 0xF, false);
}
template <typename M>
__device__ __forceinline__ M from_row_above(M v)                     // lane r <- lane r-1
{
    if constexpr (sizeof(M) == 8)
        return (M)(((uint64_t)dpp_from_above((uint32_t)(v >> 32)) << 32) | dpp_from_above((uint32_t)v));
    else
        return (M)dpp_from_above((uint32_t)v);
}
template <typename M>
__device__ __forceinline__ M from_row_below(M v)                     // lane r <- lane r+1
{
    if constexpr (sizeof(M) == 8)
        return (M)(((uint64_t)dpp_from_below((uint32_t)(v >> 32)) << 32) | dpp_from_below((uint32_t)v));
    else
        return (M)dpp_from_below((uint32_t)v);
}
// sums over the GROUP consecutive lanes that hold one board (every lane gets the result)
template <int GROUP>
__device__ __forceinline__ int group_sum(int v)
{
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <typename M>
__device__ __forceinline__ int popc(M v)
{
    if constexpr (sizeof(M) == 8) return __popcll((unsigned long long)v);
    else return __popc((uint32_t)v);
}

}  // namespace tron
