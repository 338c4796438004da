// tron_reach.hip — how far each player is from every cell (tron_reach_codes, include/tron_hip.h): k_territory's two floods
// on the same boards, keeping the level at which a cell is reached.  Out come both distance planes and eight numbers per
// board: the cells each player reaches first split by checkerboard colour, the walk bound that split allows, and each
// flood's depth.  A pure function of its arguments: no handle, nothing to invalidate.
//
//   k_reach     k_territory's layout and loop (tron_territory.hip, tron_flood.hpp): one lane per board ROW, the row a bit
//               mask, GROUP lanes per board, both floods level by level, the exit on __ballot of the frontiers, the same
//               open mask that keeps a wave shift from leaking into the neighbouring board.  Boards come in through
//               planes_in / row_masks.
//   levels      with DIST the level of every newly reached cell is kept bit-sliced: slice k of a player holds the cells
//               whose level has bit k set.  The level is the same in every lane of the wave, so `if (level >> k & 1)` is a
//               scalar branch and a level costs popcount(level) ORs per player, whatever the frontier looks like.  8 slices
//               cover sides <= 16 (at most 14 * 14 = 196 levels), 10 slices side 34 (fewer than 32 * 32 = 1 024).
//               Without DIST (out_dist == NULL) no slice exists: first_p is k_territory's own1 / own2, and the depth is
//               the last level at which a lane's row gained a cell.
//   colours     cell (r, c) has colour (r + c) & 1.  In row r the cells of head p's colour are the even columns when
//               (r ^ colour of head p) & 1 is 0, the odd ones otherwise: one of two constant masks.
//   planes out  the row lanes expand their slices to int16 in an LDS tile [2][S * S]; the tile goes out in 16-byte chunks
//               through store16, whatever the (even) address of out_dist is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tron_hip.h"
#include "tron_codes_io.hpp"
#include "tron_flood.hpp"

namespace {

using namespace tron;

constexpr int RC_BLOCK = 256;
constexpr int RC_WAVES = RC_BLOCK / 64;

// LDS of one board: with the planes wanted, the tile of 2 * G int16 in whole 16-byte chunks; then the three bit planes.
__host__ __device__ inline int tile_bytes(int G, bool dist) { return dist ? ((4 * G + 15) >> 4) << 4 : 0; }
__host__ __device__ inline int board_lds(int G, bool dist) { return (tile_bytes(G, dist) + 12 * plane_words(G) + 15) & ~15; }

template <int GROUP>
__device__ __forceinline__ int group_max(int v)
{
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// GROUP lanes per board (one lane per row), 64 / GROUP boards per wave, RC_WAVES waves per block.
template <typename M, int GROUP, bool DIST>
__global__ __launch_bounds__(RC_BLOCK) void k_reach(const int8_t *__restrict__ codes, int64_t n, int S,
                                                   int32_t *__restrict__ out_counts, int8_t *__restrict__ out_dist)
{
    extern __shared__ uint4 rc_lds[];
    constexpr int BPW = 64 / GROUP;
    constexpr int SLICES = GROUP <= 16 ? 8 : 10;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane / GROUP, row = lane % GROUP, slot = wave * BPW + grp;
    const int64_t board = (int64_t)blockIdx.x * (RC_WAVES * BPW) + slot;
    const int G = S * S;
    int8_t *tile = reinterpret_cast<int8_t *>(rc_lds) + (size_t)slot * (size_t)board_lds(G, DIST);
    uint32_t *planes = reinterpret_cast<uint32_t *>(tile + tile_bytes(G, DIST));     // [3][PW]: open, +10, -10
    const bool have = board < n;

    // ---- the board in, then my row as masks
    if (have) planes_in<GROUP>(codes, n * (int64_t)G, board * (int64_t)G, row, G, planes);
    __syncthreads();
    M inner, E, H1, H2;
    const bool playable = row_masks<M, GROUP>(planes, row, S, have && row < S, inner, E, H1, H2) && have;

    // ---- both floods, level by level; a rejected or absent board has no frontier and takes no part
    M f1 = playable ? (M)(H1 & inner) : (M)0, f2 = playable ? (M)(H2 & inner) : (M)0;
    M vis1 = f1, vis2 = f2, own1 = 0, own2 = 0;
    M lv1[SLICES], lv2[SLICES];
    if constexpr (DIST) {
#pragma unroll
        for (int k = 0; k < SLICES; ++k) lv1[k] = 0, lv2[k] = 0;
    }
    int deep1 = 0, deep2 = 0, level = 0;
    while (__ballot((f1 | f2) != 0)) {
        ++level;
        const M e1 = (M)((f1 << 1) | (f1 >> 1) | from_row_above<M>(f1) | from_row_below<M>(f1));
        const M e2 = (M)((f2 << 1) | (f2 >> 1) | from_row_above<M>(f2) | from_row_below<M>(f2));
        const M n1 = e1 & E & ~vis1, n2 = e2 & E & ~vis2;
        own1 |= n1 & ~vis2 & ~n2;
        own2 |= n2 & ~vis1 & ~n1;
        if constexpr (DIST) {
#pragma unroll
            for (int k = 0; k < SLICES; ++k)
                if ((level >> k) & 1) lv1[k] |= n1, lv2[k] |= n2;
        }
        deep1 = n1 ? level : deep1;
        deep2 = n2 ? level : deep2;
        vis1 |= n1;
        vis2 |= n2;
        f1 = n1;
        f2 = n2;
    }

    // ---- the eight counts: colour counts two to a sum (a board has at most 32 * 32 open cells), the depths by a maximum
    if (out_counts) {
        const int hc = group_sum<GROUP>(((H1 & inner) ? ((row + __ffsll((unsigned long long)(H1 & inner)) - 1) & 1) : 0)
                                        | ((H2 & inner) ? (((row + __ffsll((unsigned long long)(H2 & inner)) - 1) & 1) << 16) : 0));
        const M even = (M)0x5555555555555555ull, odd = (M)0xAAAAAAAAAAAAAAAAull;
        const M same1 = ((row ^ hc) & 1) ? odd : even, same2 = ((row ^ (hc >> 16)) & 1) ? odd : even;
        const int s1 = group_sum<GROUP>(popc<M>((M)(own1 & ~same1)) | (popc<M>((M)(own1 & same1)) << 16));
        const int s2 = group_sum<GROUP>(popc<M>((M)(own2 & ~same2)) | (popc<M>((M)(own2 & same2)) << 16));
        const int d1 = group_max<GROUP>(deep1), d2 = group_max<GROUP>(deep2);
        if (have && row < 8) {                          // opp1, same1, opp2, same2 | fill1, fill2 | depth1, depth2
            const bool second = row < 4 ? (row & 2) : (row & 1);
            const int s = second ? s2 : s1, opp = s & 0xFFFF, same = s >> 16;
            const int v = row < 4 ? ((row & 1) ? same : opp) : row < 6 ? (opp > same ? 2 * same + 1 : 2 * opp) : (second ? d2 : d1);
            out_counts[board * 8 + row] = playable ? v : -1;
        }
    }
    if constexpr (DIST) {
        // ---- the planes: a reached cell's slices to its level (0 on the head's own cell), -1 everywhere else; a rejected
        // board has reached nothing.  Then the tile out in 16-byte chunks
        if (have && row < S) {
            int16_t *t1 = reinterpret_cast<int16_t *>(tile) + row * S, *t2 = t1 + G;
            for (int c = 0; c < S; ++c) {
                int a = 0, b = 0;
#pragma unroll
                for (int k = 0; k < SLICES; ++k) {
                    a |= (int)((lv1[k] >> c) & 1) << k;
                    b |= (int)((lv2[k] >> c) & 1) << k;
                }
                t1[c] = (int16_t)(((vis1 >> c) & 1) ? a : -1);
                t2[c] = (int16_t)(((vis2 >> c) & 1) ? b : -1);
            }
        }
        __syncthreads();
        if (have) {
            const int bytes = 4 * G, chunks = (bytes + 15) >> 4;
            for (int w = row; w < chunks; w += GROUP) {
                const uint4 q = *reinterpret_cast<const uint4 *>(tile + 16 * w);
                const uint32_t x[4] = {q.x, q.y, q.z, q.w};
                store16(out_dist + board * (int64_t)bytes + 16 * w, min(16, bytes - 16 * w), x);
            }
        }
    }
}

template <typename M, int GROUP>
void launch_reach(const int8_t *codes, int64_t n, int S, int32_t *out_counts, int16_t *out_dist, hipStream_t st)
{
    constexpr int per_block = RC_WAVES * (64 / GROUP);
    const size_t smem = (size_t)per_block * (size_t)board_lds(S * S, out_dist != nullptr);   // at most 36 096 bytes (side 32, planes)
    const dim3 grid((unsigned)((n + per_block - 1) / per_block));
    int8_t *out = reinterpret_cast<int8_t *>(out_dist);
    if (out_dist) hipLaunchKernelGGL((k_reach<M, GROUP, true>), grid, dim3(RC_BLOCK), smem, st, codes, n, S, out_counts, out);
    else hipLaunchKernelGGL((k_reach<M, GROUP, false>), grid, dim3(RC_BLOCK), smem, st, codes, n, S, out_counts, out);
}

}  // namespace

extern "C" int tron_reach_codes(const int8_t *codes, int64_t n, int32_t side, int32_t *out_counts, int16_t *out_dist,
                                void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || (!codes && n > 0)) return TRON_ERR_BAD_ARG;
    if (out_dist && ((reinterpret_cast<uintptr_t>(out_dist) & 1u) || reinterpret_cast<const int8_t *>(out_dist) == codes))
        return TRON_ERR_BAD_ARG;
    if (side < 6 || side > 34) return TRON_ERR_UNSUPPORTED;
    if (n == 0 || (!out_counts && !out_dist)) return TRON_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (side <= 8) launch_reach<uint32_t, 8>(codes, n, side, out_counts, out_dist, st);
    else if (side <= 16) launch_reach<uint32_t, 16>(codes, n, side, out_counts, out_dist, st);
    else if (side <= 32) launch_reach<uint32_t, 32>(codes, n, side, out_counts, out_dist, st);
    else launch_reach<uint64_t, 64>(codes, n, side, out_counts, out_dist, st);
    return hipGetLastError() == hipSuccess ? TRON_OK : TRON_ERR_LAUNCH;
}
