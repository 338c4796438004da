// tron_territory.hip — who reaches which cell first (tron_territory_codes, include/tron_hip.h): for every board of a stack
// of observation-code images, both players' breadth-first floods over the open cells, counted and, if asked for, written
// out as an owner plane.  A pure function of its arguments: no handle, nothing to invalidate.
//
//   k_territory   the layout voronoi() in tron_minimax.hip proves out: one lane per board ROW, the row a bit mask (bit c =
//               column c), GROUP lanes per board and 64 / GROUP boards per wave.  Both floods advance level by level —
//               left / right are shifts within the mask, up / down one DPP wave shift each (tron_flood.hpp) — and every
//               newly reached cell is classified on the spot into one of three masks: reached by player 1 first, by
//               player 2 first, by both at the same level.  The loop leaves on __ballot of the frontiers, so a wave runs
//               as many levels as its deepest board needs.
//   the leak    a wave shift carries a row into the neighbouring board's lanes.  What stops it is the OPEN mask, not the
//               data: a board's row 0 and row S - 1 (and every lane behind row S - 1) have an open mask of 0 and columns 0
//               and S - 1 are cleared in every row, whatever bytes the caller's border ring holds.  A frontier is always
//               a subset of the open mask (the heads' start bits are strictly inside too: a board whose head is not is
//               rejected and floods nothing), so a board's first and last lane never hold a frontier bit and the
//               neighbouring board is handed zeros.
//   boards in   as the playouts bring them in (load16, tron_codes_io.hpp): 16-byte
//               aligned chunks put together with v_alignbyte whatever a board's base address is; a chunk that sticks out
//               of the caller's buffer is read byte by byte inside it.  A chunk becomes 16 bits in each of three bit
//               planes in LDS (open, +10, -10), and a row lane takes its S bits out of three consecutive words.
//   owner out   the row lanes expand their masks to bytes in an LDS tile; the tile goes out in 16-byte chunks, one 16-byte
//               store where the address allows it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tron_hip.h"
#include "tron_codes_io.hpp"
#include "tron_flood.hpp"

namespace {

using namespace tron;

constexpr int TT_BLOCK = 256;
constexpr int TT_WAVES = TT_BLOCK / 64;

// LDS of one board: the owner tile (S * S bytes in whole 16-byte chunks), then the three bit planes of `plane_words` words.
__host__ __device__ inline int board_lds(int G) { return ((((G + 15) >> 4) << 4) + 12 * plane_words(G) + 15) & ~15; }

// GROUP lanes per board (one lane per row), 64 / GROUP boards per wave, TT_WAVES waves per block.
template <typename M, int GROUP>
__global__ __launch_bounds__(TT_BLOCK) void k_territory(const int8_t *__restrict__ codes, int64_t n, int S,
                                                       int32_t *__restrict__ out_counts, int8_t *__restrict__ out_owner)
{
    extern __shared__ uint4 tt_lds[];
    constexpr int BPW = 64 / GROUP;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane / GROUP, row = lane % GROUP, slot = wave * BPW + grp;
    const int64_t board = (int64_t)blockIdx.x * (TT_WAVES * BPW) + slot;
    const int G = S * S, CHUNKS = (G + 15) >> 4;
    int8_t *tile = reinterpret_cast<int8_t *>(tt_lds) + (size_t)slot * (size_t)board_lds(G);
    uint32_t *planes = reinterpret_cast<uint32_t *>(tile + CHUNKS * 16);      // [3][PW]: open, +10, -10
    const bool have = board < n;
    const int64_t total = n * (int64_t)G, base = board * (int64_t)G;

    // ---- the board in, then my row as masks
    if (have) planes_in<GROUP>(codes, total, base, row, G, planes);
    __syncthreads();
    M inner, E, H1, H2;
    const bool playable = row_masks<M, GROUP>(planes, row, S, have && row < S, inner, E, H1, H2) && have;

    // ---- both floods, level by level; a rejected or absent board has no frontier and takes no part
    M f1 = playable ? (M)(H1 & inner) : (M)0, f2 = playable ? (M)(H2 & inner) : (M)0;
    M vis1 = f1, vis2 = f2, own1 = 0, own2 = 0, tied = 0;
    while (__ballot((f1 | f2) != 0)) {
        const M e1 = (M)((f1 << 1) | (f1 >> 1) | from_row_above<M>(f1) | from_row_below<M>(f1));
        const M e2 = (M)((f2 << 1) | (f2 >> 1) | from_row_above<M>(f2) | from_row_below<M>(f2));
        const M n1 = e1 & E & ~vis1, n2 = e2 & E & ~vis2;
        own1 |= n1 & ~vis2 & ~n2;
        own2 |= n2 & ~vis1 & ~n1;
        tied |= n1 & n2;
        vis1 |= n1;
        vis2 |= n2;
        f1 = n1;
        f2 = n2;
    }

    // ---- the six counts, two to a sum (a board has at most 32 * 32 open cells)
    if (out_counts) {
        const int s01 = group_sum<GROUP>(popc<M>(own1) | (popc<M>(own2) << 16));
        const int s23 = group_sum<GROUP>(popc<M>(tied) | (popc<M>((M)(E & ~vis1 & ~vis2)) << 16));
        const int s45 = group_sum<GROUP>(popc<M>((M)(E & vis1)) | (popc<M>((M)(E & vis2)) << 16));
        if (have && row < 6) {
            const int s = row < 2 ? s01 : row < 4 ? s23 : s45;
            out_counts[board * 6 + row] = playable ? ((row & 1) ? (s >> 16) : (s & 0xFFFF)) : -1;
        }
    }
    if (!out_owner) return;

    // ---- the owner plane: rows to bytes in the tile, the tile out in 16-byte chunks
    if (have && row < S) {
        int8_t *tr = tile + row * S;
        for (int c = 0; c < S; ++c)
            tr[c] = (int8_t)(((own1 >> c) & 1) | (((own2 >> c) & 1) << 1) | (((tied >> c) & 1) * 3));
    }
    __syncthreads();
    if (have) {
        for (int w = row; w < CHUNKS; w += GROUP) {
            const uint4 q = *reinterpret_cast<const uint4 *>(tile + 16 * w);
            const uint32_t x[4] = {q.x, q.y, q.z, q.w};
            store16(out_owner + base + 16 * w, min(16, G - 16 * w), x);
        }
    }
}

template <typename M, int GROUP>
void launch_territory(const int8_t *codes, int64_t n, int S, int32_t *out_counts, int8_t *out_owner, hipStream_t st)
{
    constexpr int per_block = TT_WAVES * (64 / GROUP);
    const size_t smem = (size_t)per_block * (size_t)board_lds(S * S);          // 6 592 bytes at side 34, 11 520 at side 32
    const dim3 grid((unsigned)((n + per_block - 1) / per_block));
    hipLaunchKernelGGL((k_territory<M, GROUP>), grid, dim3(TT_BLOCK), smem, st, codes, n, S, out_counts, out_owner);
}

}  // namespace

extern "C" int tron_territory_codes(const int8_t *codes, int64_t n, int32_t side, int32_t *out_counts, int8_t *out_owner,
                                    void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || (!codes && n > 0) || (out_owner && out_owner == codes)) return TRON_ERR_BAD_ARG;
    if (side < 6 || side > 34) return TRON_ERR_UNSUPPORTED;
    if (n == 0 || (!out_counts && !out_owner)) return TRON_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (side <= 8) launch_territory<uint32_t, 8>(codes, n, side, out_counts, out_owner, st);
    else if (side <= 16) launch_territory<uint32_t, 16>(codes, n, side, out_counts, out_owner, st);
    else if (side <= 32) launch_territory<uint32_t, 32>(codes, n, side, out_counts, out_owner, st);
    else launch_territory<uint64_t, 64>(codes, n, side, out_counts, out_owner, st);
    return hipGetLastError() == hipSuccess ? TRON_OK : TRON_ERR_LAUNCH;
}
