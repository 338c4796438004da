// tron_search.hip — exact maximin move values one to three plies deep (tron_search_codes, include/tron_hip.h): for every
// board of a stack of observation-code images, every joint line of PLIES simultaneous moves under mode None's step rule,
// the territory difference at the leaves, and a separate maximin for each player.  Integers only, one launch.  A pure
// function of its arguments: no handle, nothing to invalidate.
//
//   k_search    k_moves' and k_reach's layout (tron_moves.hip, tron_reach.hip, tron_flood.hpp): one lane per board ROW, the
//               row a bit mask, GROUP lanes per board, boards in through planes_in / row_masks.
//   the tree    walked as k_minimax walks its own: all boards of a wave go through the 16 joint moves of a node together,
//               and a board predicates away the lines it does not have.  A position is three masks (E, H1, H2); a target
//               is the head's bit shifted within the row or handed to the row above / below; the child is E without the
//               two targets and the targets as heads.  A board that does not go down a line hands its child empty heads:
//               every move below is unsafe there, nothing floods, and what the subtree returns for it is not used.
//   one level   node<R, K> is one level with R plies left after K joint moves; the levels are template instances inlined
//               into each other, so each level's masks, targets and folds are scalars and arrays under constant indices
//               in registers.  The loop over the 16 joint moves is rolled (its counter is wave-uniform); nothing is
//               indexed by it: the target and the fold slot are chosen by selects.
//   safety      eight safe bits and sixteen same-cell bits of a node go through ONE group_or: each is set in at most one
//               lane of a board.
//   the skip    a joint move no board of the wave plays on (not both targets safe and distinct) is decided from those
//               bits alone: the subtree under it is not entered.  Terminals need no flood.
//   the leaf    voronoi()'s two-front flood (tron_minimax.hip) counting first1 - first2 only, one group_sum; the exit on
//               __ballot keeps a finished board's frontier empty while its neighbours go on.
//   the fold    min over the opponent's move, max over the own, for both players, in every lane of the board; lanes 0..7
//               write the eight root values, lanes 0 and 1 the picks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tron_hip.h"
#include "tron_codes_io.hpp"
#include "tron_flood.hpp"

namespace {

using namespace tron;

constexpr int SR_BLOCK = 256;
constexpr int SR_WAVES = SR_BLOCK / 64;
constexpr int SR_DECIDED = 2048;                                       // a line decided after k joint moves is worth 2048 - k
constexpr int32_t SR_REJECTED = INT32_MIN;

// ORs over the GROUP consecutive lanes that hold one board (every lane gets the result)
template <int GROUP>
__device__ __forceinline__ int group_or(int v)
{
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// the four cells beside a head, each in the lane of its row: UP is handed to the row above, DOWN to the row below
template <typename M>
__device__ __forceinline__ void targets(M H, M (&t)[4])
{
    t[0] = from_row_below<M>(H);
    t[1] = (M)(H << 1);
    t[2] = from_row_above<M>(H);
    t[3] = (M)(H >> 1);
}
template <typename T>
__device__ __forceinline__ T pick4(const T (&v)[4], int i)             // i is wave-uniform
{
    return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
}
__device__ __forceinline__ int max4(const int (&v)[4])
{
    const int x = v[0] > v[1] ? v[0] : v[1], y = v[2] > v[3] ? v[2] : v[3];
    return x > y ? x : y;
}

// first1 - first2 of the position (open, heads f1 / f2); a board with empty heads floods nothing and gets 0
template <typename M, int GROUP>
__device__ __forceinline__ int leaf(M open, M f1, M f2)
{
    M vis1 = f1, vis2 = f2;
    int acc = 0;
    while (__ballot((f1 | f2) != 0)) {
        const M n1 = spread<M>(f1) & open & ~vis1, n2 = spread<M>(f2) & open & ~vis2;
        acc += popc<M>((M)(n1 & ~vis2 & ~n2)) - popc<M>((M)(n2 & ~vis1 & ~n1));
        vis1 |= n1;
        vis2 |= n2;
        f1 = n1;
        f2 = n2;
    }
    return group_sum<GROUP>(acc);
}

// U_1(a) and U_2(b) of the node (E, H1, H2) with R plies left, reached after K joint moves.  A board with empty heads gets
// zeros.
template <typename M, int GROUP, int R, int K>
__device__ __forceinline__ void node(M E, M H1, M H2, int (&u1)[4], int (&u2)[4])
{
    M t1[4], t2[4];
    targets<M>(H1, t1);
    targets<M>(H2, t2);
    int bits = 0;                                                      // bit a: T_1(a) safe, 4 + b: T_2(b) safe, 8 + 4a + b: same cell
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        bits |= ((t1[a] & E) ? 1 << a : 0) | ((t2[a] & E) ? 16 << a : 0);
#pragma unroll
        for (int b = 0; b < 4; ++b) bits |= (t1[a] & t2[b]) ? 256 << (4 * a + b) : 0;
    }
    bits = group_or<GROUP>(bits);
#pragma unroll
    for (int k = 0; k < 4; ++k) u1[k] = u2[k] = INT32_MAX;
#pragma unroll 1
    for (int ab = 0; ab < 16; ++ab) {
        const int a = ab >> 2, b = ab & 3;
        const bool s1 = (bits >> a) & 1, s2 = (bits >> (4 + b)) & 1;
        const bool on = s1 && s2 && !((bits >> (8 + ab)) & 1);         // the line goes on: both safe, two cells
        int w1 = s1 == s2 ? 0 : s1 ? SR_DECIDED - K : K - SR_DECIDED, w2 = -w1;
        if (__ballot(on)) {
            const M c1 = on ? pick4<M>(t1, a) : (M)0, c2 = on ? pick4<M>(t2, b) : (M)0;
            const M open = E & ~c1 & ~c2;
            int v1, v2;
            if constexpr (R == 1) {
                v1 = leaf<M, GROUP>(open, c1, c2);
                v2 = -v1;
            } else {
                int d1[4], d2[4];
                node<M, GROUP, R - 1, K + 1>(open, c1, c2, d1, d2);
                v1 = max4(d1);
                v2 = max4(d2);
            }
            w1 = on ? v1 : w1;
            w2 = on ? v2 : w2;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u1[k] = (k == a && w1 < u1[k]) ? w1 : u1[k];
            u2[k] = (k == b && w2 < u2[k]) ? w2 : u2[k];
        }
    }
}

// GROUP lanes per board (one lane per row), 64 / GROUP boards per wave, SR_WAVES waves per block.
template <typename M, int GROUP, int PLIES>
__global__ __launch_bounds__(SR_BLOCK) void k_search(const int8_t *__restrict__ codes, int64_t n, int S,
                                                    int32_t *__restrict__ out_values, int8_t *__restrict__ out_actions)
{
    extern __shared__ uint4 sr_lds[];
    constexpr int BPW = 64 / GROUP;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int grp = lane / GROUP, row = lane % GROUP, slot = wave * BPW + grp;
    const int64_t board = (int64_t)blockIdx.x * (SR_WAVES * BPW) + slot;
    const int G = S * S;
    uint32_t *planes = reinterpret_cast<uint32_t *>(reinterpret_cast<int8_t *>(sr_lds) + (size_t)slot * (size_t)planes_lds(G));
    const bool have = board < n;

    // ---- the board in, then my row as masks; a rejected or absent board has no heads
    if (have) planes_in<GROUP>(codes, n * (int64_t)G, board * (int64_t)G, row, G, planes);
    __syncthreads();
    M inner, E, H1, H2;
    const bool playable = row_masks<M, GROUP>(planes, row, S, have && row < S, inner, E, H1, H2) && have;
    H1 = playable ? (M)(H1 & inner) : (M)0;
    H2 = playable ? (M)(H2 & inner) : (M)0;

    // ---- the tree
    int u1[4], u2[4];
    node<M, GROUP, PLIES, 0>(E, H1, H2, u1, u2);
    if (!have || row >= 8) return;

    // ---- lane `row` of the board writes value row = p * 4 + a; lanes 0 and 1 pick for player 0 and 1
    if (out_values) {
        int mine = u1[0];
#pragma unroll
        for (int f = 1; f < 8; ++f) mine = row == f ? (f < 4 ? u1[f & 3] : u2[f & 3]) : mine;
        out_values[board * 8 + row] = playable ? mine : SR_REJECTED;
    }
    if (out_actions && row < 2) {
        int best = 0, top = row ? u2[0] : u1[0];
#pragma unroll
        for (int a = 1; a < 4; ++a) {
            const int v = row ? u2[a] : u1[a];
            if (v > top) best = a, top = v;
        }
        out_actions[board * 2 + row] = (int8_t)(playable ? best : -1);
    }
}

template <typename M, int GROUP>
void launch_search(const int8_t *codes, int64_t n, int S, int plies, int32_t *out_values, int8_t *out_actions, hipStream_t st)
{
    constexpr int per_block = SR_WAVES * (64 / GROUP);
    const size_t smem = (size_t)per_block * (size_t)planes_lds(S * S);         // at most 3 328 bytes (side 32)
    const dim3 grid((unsigned)((n + per_block - 1) / per_block));
    if (plies == 1)
        hipLaunchKernelGGL((k_search<M, GROUP, 1>), grid, dim3(SR_BLOCK), smem, st, codes, n, S, out_values, out_actions);
    else if (plies == 2)
        hipLaunchKernelGGL((k_search<M, GROUP, 2>), grid, dim3(SR_BLOCK), smem, st, codes, n, S, out_values, out_actions);
    else
        hipLaunchKernelGGL((k_search<M, GROUP, 3>), grid, dim3(SR_BLOCK), smem, st, codes, n, S, out_values, out_actions);
}

}  // namespace

extern "C" int tron_search_codes(const int8_t *codes, int64_t n, int32_t side, int32_t plies, int32_t *out_values,
                                 int8_t *out_actions, void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || (!codes && n > 0)) return TRON_ERR_BAD_ARG;
    if (side < 6 || side > 34 || plies < 1 || plies > 3) return TRON_ERR_UNSUPPORTED;
    if (n == 0 || (!out_values && !out_actions)) return TRON_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (side <= 8) launch_search<uint32_t, 8>(codes, n, side, plies, out_values, out_actions, st);
    else if (side <= 16) launch_search<uint32_t, 16>(codes, n, side, plies, out_values, out_actions, st);
    else if (side <= 32) launch_search<uint32_t, 32>(codes, n, side, plies, out_values, out_actions, st);
    else launch_search<uint64_t, 64>(codes, n, side, plies, out_values, out_actions, st);
    return hipGetLastError() == hipSuccess ? TRON_OK : TRON_ERR_LAUNCH;
}
