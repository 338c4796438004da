// tron_moves.hip — what each move leads into (tron_moves_codes, include/tron_hip.h): for every board of a stack of
// observation-code images and each of the up to eight safe move targets, the room behind the target, the checkerboard
// bound on the moves it can hold, and how much of it the mover still reaches before the opponent once the step is spent;
// and the pick those numbers make.  A pure function of its arguments: no handle, nothing to invalidate.
//
//   k_moves     k_reach's layout and loop (tron_reach.hip, tron_flood.hpp): one lane per board ROW, the row a bit mask,
//               GROUP lanes per board, the exit on __ballot of the frontiers, the open mask that keeps a wave shift from
//               leaking into the neighbouring board.  Boards come in through planes_in / row_masks.
//   ten floods  flood p * 4 + a starts on player p's target in direction a, floods 8 and 9 on the heads; all ten run on
//               one clock.  At time 1 a target frontier is the single bit t & E — the head's bit shifted within the row or
//               handed to the row above / below — and a head frontier the head's open neighbours, which is the OR of that
//               player's four target bits.  At every later time each frontier advances one level.  A target flood's cell
//               of time T has e = T - 1, so the mover stands on it at 1 + e = T, and the opponent's head flood holds after
//               time T exactly the cells with d_q <= T: `first` gathers new & ~vis_q with vis_q taken after q's cells of
//               the same time are in.  A target the opponent also stands beside (d_q = 1) drops out at time 1 by itself.
//   registers   frontiers, visited and first masks are arrays under constant indices in unrolled loops: 28 masks, no
//               scratch.  No level is stored: room, same and opp come from the final visited masks and two constant
//               colour masks.
//   counts      a board has at most 32 * 32 - 2 open cells, at most 512 of either colour, so same (10 bits), opp (10 bits)
//               and first (12 bits) of a flood go into ONE group_sum; room = same + opp.
//   the pick    every lane of a board holds all eight sums; the two lanes that write out_actions compare
//               first * 2048 + fill (fill <= 1 024) of their player's four moves, -1 for an unsafe one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tron_hip.h"
#include "tron_codes_io.hpp"
#include "tron_flood.hpp"

namespace {

using namespace tron;

constexpr int MV_BLOCK = 256;
constexpr int MV_WAVES = MV_BLOCK / 64;

// spread(): the cells a frontier reaches in one level, walls and all (tron_flood.hpp)
// GROUP lanes per board (one lane per row), 64 / GROUP boards per wave, MV_WAVES waves per block.
template <typename M, int GROUP>
__global__ __launch_bounds__(MV_BLOCK) void k_moves(const int8_t *__restrict__ codes, int64_t n, int S,
                                                   int32_t *__restrict__ out_moves, int8_t *__restrict__ out_actions)
{
    extern __shared__ uint4 mv_lds[];
    constexpr int BPW = 64 / GROUP;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane / GROUP, row = lane % GROUP, slot = wave * BPW + grp;
    const int64_t board = (int64_t)blockIdx.x * (MV_WAVES * BPW) + slot;
    const int G = S * S;
    uint32_t *planes = reinterpret_cast<uint32_t *>(reinterpret_cast<int8_t *>(mv_lds) + (size_t)slot * (size_t)planes_lds(G));
    const bool have = board < n;

    // ---- the board in, then my row as masks
    if (have) planes_in<GROUP>(codes, n * (int64_t)G, board * (int64_t)G, row, G, planes);
    __syncthreads();
    M inner, E, H1, H2;
    const bool playable = row_masks<M, GROUP>(planes, row, S, have && row < S, inner, E, H1, H2) && have;

    // ---- time 1: the eight target bits and the heads' open neighbours; a rejected or absent board has no frontier
    M fr[10], vis[10], fst[8];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const M H = playable ? (M)((p ? H2 : H1) & inner) : (M)0;
        fr[4 * p + 0] = from_row_below<M>(H) & E;                      // UP: the row above me takes my bit
        fr[4 * p + 1] = (M)(H << 1) & E;                               // RIGHT
        fr[4 * p + 2] = from_row_above<M>(H) & E;                      // DOWN
        fr[4 * p + 3] = (M)(H >> 1) & E;                               // LEFT
        fr[8 + p] = fr[4 * p] | fr[4 * p + 1] | fr[4 * p + 2] | fr[4 * p + 3];
    }
#pragma unroll
    for (int f = 0; f < 10; ++f) vis[f] = fr[f];
#pragma unroll
    for (int f = 0; f < 8; ++f) fst[f] = fr[f] & ~vis[9 - (f >> 2)];

    // ---- every later time: all ten one level on, the heads first
    M any = fr[8] | fr[9];
    while (__ballot(any != 0)) {
        any = 0;
#pragma unroll
        for (int f = 9; f >= 0; --f) {
            const M nw = spread<M>(fr[f]) & E & ~vis[f];
            vis[f] |= nw;
            fr[f] = nw;
            any |= nw;
            if (f < 8) fst[f] |= nw & ~vis[9 - (f >> 2)];
        }
    }

    // ---- same | opp << 10 | first << 20 of every move, one sum each.  The targets of head p have the colour head p has
    // not: in row r that is the odd columns when (r ^ colour of head p) & 1 is 0
    const int hc = group_sum<GROUP>(((H1 & inner) ? ((row + __ffsll((unsigned long long)(H1 & inner)) - 1) & 1) : 0)
                                    | ((H2 & inner) ? (((row + __ffsll((unsigned long long)(H2 & inner)) - 1) & 1) << 16) : 0));
    const M even = (M)0x5555555555555555ull, odd = (M)0xAAAAAAAAAAAAAAAAull;
    int sums[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        const M same = ((row ^ (f < 4 ? hc : (hc >> 16))) & 1) ? even : odd;
        sums[f] = group_sum<GROUP>(popc<M>((M)(vis[f] & same)) | (popc<M>((M)(vis[f] & ~same)) << 10) | (popc<M>(fst[f]) << 20));
    }
    if (!have || row >= 8) return;

    // ---- lane `row` of the board writes move row = p * 4 + a; lanes 0 and 1 pick for player 0 and 1
    int mine = 0, key[4];
#pragma unroll
    for (int f = 0; f < 8; ++f) mine = row == f ? sums[f] : mine;
    if (out_moves) {
        const int same = mine & 0x3FF, opp = (mine >> 10) & 0x3FF, room = same + opp;
        int32_t *o = out_moves + board * 24 + row * 3;
        o[0] = room ? room : -1;
        o[1] = room ? (same > opp ? 2 * opp + 1 : 2 * same) : -1;
        o[2] = room ? (int)((uint32_t)mine >> 20) : -1;
    }
    if (out_actions && row < 2) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int s = row ? sums[4 + a] : sums[a];
            const int same = s & 0x3FF, opp = (s >> 10) & 0x3FF;
            key[a] = same + opp ? (int)((uint32_t)s >> 20) * 2048 + (same > opp ? 2 * opp + 1 : 2 * same) : -1;
        }
        int best = 0, top = key[0];
#pragma unroll
        for (int a = 1; a < 4; ++a)
            if (key[a] > top) best = a, top = key[a];
        out_actions[board * 2 + row] = (int8_t)(playable ? best : -1);
    }
}

template <typename M, int GROUP>
void launch_moves(const int8_t *codes, int64_t n, int S, int32_t *out_moves, int8_t *out_actions, hipStream_t st)
{
    constexpr int per_block = MV_WAVES * (64 / GROUP);
    const size_t smem = (size_t)per_block * (size_t)planes_lds(S * S);          // at most 3 328 bytes (side 32)
    const dim3 grid((unsigned)((n + per_block - 1) / per_block));
    hipLaunchKernelGGL((k_moves<M, GROUP>), grid, dim3(MV_BLOCK), smem, st, codes, n, S, out_moves, out_actions);
}

}  // namespace

extern "C" int tron_moves_codes(const int8_t *codes, int64_t n, int32_t side, int32_t *out_moves, int8_t *out_actions,
                                void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || (!codes && n > 0)) return TRON_ERR_BAD_ARG;
    if (side < 6 || side > 34) return TRON_ERR_UNSUPPORTED;
    if (n == 0 || (!out_moves && !out_actions)) return TRON_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (side <= 8) launch_moves<uint32_t, 8>(codes, n, side, out_moves, out_actions, st);
    else if (side <= 16) launch_moves<uint32_t, 16>(codes, n, side, out_moves, out_actions, st);
    else if (side <= 32) launch_moves<uint32_t, 32>(codes, n, side, out_moves, out_actions, st);
    else launch_moves<uint64_t, 64>(codes, n, side, out_moves, out_actions, st);
    return hipGetLastError() == hipSuccess ? TRON_OK : TRON_ERR_LAUNCH;
}
