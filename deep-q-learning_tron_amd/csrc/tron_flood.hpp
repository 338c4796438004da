// tron_flood.hpp — what the level-synchronous bitboard floods share (tron_minimax.hip's voronoi(),
// tron_territory.hip, tron_reach.hip).  One lane per board ROW, the row a bit mask (bit c = column c): left / right are
// shifts within the mask, up / down one whole-wave DPP shift each.  The second half is how the two kernels that flood
// observation-code boards (k_territory, k_reach) bring a board in and turn it into row masks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tron_codes_io.hpp"

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
// the cells a frontier reaches in one level, walls and all (k_moves, k_search)
template <typename M>
__device__ __forceinline__ M spread(M f)
{
    return (M)((f << 1) | (f >> 1) | from_row_above<M>(f) | from_row_below<M>(f));
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

// ---- observation-code boards as row masks (k_territory, k_reach) -----------------------------------------------------
// A board comes in as load16 brings it (tron_codes_io.hpp): chunk w of the board becomes 16 bits in each of three bit
// planes in LDS (open, +10, -10; bit i of the board = bit i & 31 of word i >> 5), and a row lane takes its S bits out of
// three consecutive words of a plane.
// Words of one plane of a board of G cells: the cells, and two words of slack behind the last one for row_bits.
__host__ __device__ inline int plane_words(int G) { return ((G + 31) >> 5) + 2; }
// LDS of a board that is held as its three bit planes and nothing else (k_moves, k_search), a multiple of 16 bytes.
__host__ __device__ inline int planes_lds(int G) { return (12 * plane_words(G) + 15) & ~15; }

// Bits [start, start + S) of a bit plane, S <= 34: three words cover them wherever they start.
template <typename M>
__device__ __forceinline__ M row_bits(const uint32_t *plane, int start, int S)
{
    const int k = start >> 5, off = start & 31;
    uint64_t v = (((uint64_t)plane[k + 1] << 32) | plane[k]) >> off;
    if (off) v |= (uint64_t)plane[k + 2] << (64 - off);
    return (M)(v & ((1ull << S) - 1ull));
}

// The board of G cells at codes[base, base + G) (codes holds `total` bytes) into planes[3][plane_words(G)], by the GROUP
// lanes of the board, lane `row` taking every GROUP-th chunk.  The caller's __syncthreads() comes before the planes are read.
template <int GROUP>
__device__ __forceinline__ void planes_in(const int8_t *__restrict__ codes, int64_t total, int64_t base, int row, int G,
                                          uint32_t *planes)
{
    const int CHUNKS = (G + 15) >> 4, PW = plane_words(G);
    uint16_t *halves = reinterpret_cast<uint16_t *>(planes);
    for (int w = row; w < CHUNKS; w += GROUP) {
        uint32_t x[4];
        load16(codes, total, base + 16 * w, x);
        uint32_t open = 0u, h1 = 0u, h2 = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int v = (int)(int8_t)(x[i >> 2] >> (8 * (i & 3)));          // bytes behind the board's end belong to no row
            open |= (uint32_t)(v == 1) << i;
            h1 |= (uint32_t)(v == 10) << i;
            h2 |= (uint32_t)(v == -10) << i;
        }
        halves[w] = (uint16_t)open;
        halves[2 * PW + w] = (uint16_t)h1;
        halves[4 * PW + w] = (uint16_t)h2;
    }
}

// Row `row` of a board of side S out of its planes: E the open cells (byte 1, strictly inside the border: nothing outside
// `inner` is ever open), H1 / H2 the +10 / -10 bytes of the whole row.  Returns whether the board is playable: exactly
// one +10 and one -10 on the whole image, both strictly inside the border.  A lane with `mine` false (no board, or a
// lane behind row S - 1) holds zeros and takes part in the sums.
template <typename M, int GROUP>
__device__ __forceinline__ bool row_masks(const uint32_t *planes, int row, int S, bool mine, M &inner, M &E, M &H1, M &H2)
{
    const int PW = plane_words(S * S);
    inner = (row >= 1 && row <= S - 2) ? (M)((((M)1 << (S - 2)) - (M)1) << 1) : (M)0;
    E = 0, H1 = 0, H2 = 0;
    if (mine) {
        E = row_bits<M>(planes, row * S, S) & inner;
        H1 = row_bits<M>(planes + PW, row * S, S);
        H2 = row_bits<M>(planes + 2 * PW, row * S, S);
    }
    const int all = group_sum<GROUP>(popc<M>(H1) | (popc<M>(H2) << 16));
    const int in = group_sum<GROUP>(popc<M>(H1 & inner) | (popc<M>(H2 & inner) << 16));
    return all == 0x00010001 && in == 0x00010001;
}

}  // namespace tron
