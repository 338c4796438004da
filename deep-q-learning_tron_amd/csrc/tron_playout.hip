// Stateless batched playouts from observation-code boards (tron_playout_codes, include/tron_hip.h): every board is played
// forward up to K steps under mode None's rule (Game.step, game.py:149-277) with no restart, and the call reports how it
// ended.  A pure function of its arguments: no handle, nothing to invalidate.
//
//   k_playout   one lane per playout, one wave per workgroup.  A lane's board is packed two bits per cell in LDS, word w
//               of lane l at [w * 64 + l]: whatever cell a lane touches, its bank is its lane number, so the step loop has
//               no bank conflict.  The board is the reference's grid at the moment moves are judged — after both heads
//               have turned into bodies (game.py:155-156) — so a head's cell holds its owner's trail; the heads
//               themselves, the alive bits and the step count are registers.  A step costs two LDS reads and two LDS
//               writes, a drawn move four reads more per player.
//               Boards come in and go out through groups of four lanes per board (64-byte runs of global memory, a
//               four-way bank conflict in LDS; sixteen boards per instruction).  Reads are 16-byte aligned chunks put
//               together with v_alignbyte, whatever a board's base address is (odd sides, sliced tensors); only a chunk
//               that sticks out of the caller's buffer is read byte by byte.
// tron_playout_values fans every board out over the 16 joint first moves and tallies the endings: k_playout_values and
// k_values_pick below, made of the same board-in, start and step functions as k_playout.
//
// tron_playout_slide_codes / tron_playout_slide_values play the sliding rule of "ice" and "temper" (one slide rate per
// player and board): k_playout_slide and k_playout_values_slide are the two kernel bodies above instantiated with
// playout_step_slide in the place of playout_step — same lanes, same LDS column, same phases before and behind the steps;
// the mode-None kernels are the instantiations without it and compile to what they were.
//   the sliding step   can look at four cells: each player's target n[p] and the cell behind it, sl[p], where a slide
//               lands.  All four addresses follow from the heads and the moves alone (sl[p] = n[p] when the target is
//               off the interior, so no address leaves the image), so all four are read in ONE round trip, before
//               anything is decided, as lane_move does for the env (tron_env.hip).  What a later read of the reference
//               would see of an earlier write of the same step — player 1's slide tile on player 2's target or landing,
//               player 2's slide tile on player 1's new cell, player 1's head on player 2's — is a comparison of cell
//               indices in registers.  A drawn move's four neighbours are a round trip of their own before that, as in
//               the mode-None step: two round trips per drawn step in either rule.
//               The up to four cells a step fills (two slide tiles, two trails under the new heads) go out as ds_or
//               without return, in program order: no read-modify-write, so words that coincide need no care.  A slide
//               tile is only ever laid on an EMPTY cell, so the OR is the cell's value; a trail ORed onto a cell that
//               was not EMPTY belongs to a player that died there, the playout ends, and the head byte covers the cell.
//   the decision       is (double)u <= rate as the reference writes it, on the lane's two float64 rates (four VGPRs): one
//               conversion and one compare per player and step, exact for every float and every double (NaN, negative
//               and >= 1 rates included) with no threshold to derive.  u comes from the caller's tape, or from words 2
//               and 3 of the step's Philox block by the env's conversion; without a tape the block is drawn every step.
//
// tron_playout_weighted_codes / tron_playout_weighted_values replace the uniform safe draw by one that weighs every safe
// move by its room (include/tron_hip.h): the four kernel bodies above instantiated once more with WEIGHTED, in which
// playout_step and playout_step_slide — still the only copies of the rule — take a drawn move from safe_move_weighted
// instead of safe_move.  The instantiations without it compile to what they were; the four weights are one uint32 kernel
// argument, wave-uniform, in an SGPR.
//   the weighted draw  looks at the twelve cells within two steps of the head: the
//               four targets, the four diagonals (each a neighbour of two targets) and the four cells two steps on in a
//               straight line (a neighbour of one).  The head is strictly inside the border (playout_start; a player
//               that left the interior has died and the playout is over), so the targets and the diagonals lie in the
//               side x side image whatever the board holds.  The cell two steps on lies in it exactly when its target is
//               strictly inside the border, which is register arithmetic on the head's coordinates (on_board), not a
//               property of the board: where it is not, the target's own address is read in its place and the result
//               is discarded.  So every address is inside the lane's own column for any board a caller can pass — a
//               border cell that reads EMPTY included — and, as none depends on a cell's value, all twelve reads are
//               ONE round trip in the place of safe_move's four: two round trips per drawn step, as before.  A lane's
//               cells live in its own bank, so nothing conflicts.
//               The pick is branch-free: w[a] = byte k(a) of the weights for a safe move and 0 otherwise; if they sum to
//               0 every safe move weighs 1 (the uniform rule is the same running-sum pick); the move is the number of
//               running sums that mulhi(u, sum) has reached.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tron_hip.h"
#include "tron_codes_io.hpp"
#include "tron_device.hpp"

namespace {

using namespace tron;

constexpr int PO_LANES = 64;                       // playouts per workgroup: one wave
constexpr int PO_GROUP = 4;                        // lanes that share a board while boards are loaded and stored
constexpr int PO_BOARDS = PO_LANES / PO_GROUP;     // boards per load / store instruction
// a cell's two bits; PO_P1_HEAD is never stored: it is what plain_targets hands player 2 on player 1's new head
constexpr uint32_t PO_EMPTY = 0u, PO_P1 = 1u, PO_P2 = 2u, PO_WALL = 3u, PO_P1_HEAD = 4u;
constexpr uint32_t PO_COPY = 0x80000000u;          // info word of the store phase: this board's output is its input

// Heads seen so far in a board, 16 bits per player: how many (0, 1, 2 = more than one) | the first one's cell << 2.
__device__ __forceinline__ uint32_t head_seen(uint32_t heads, int p, int cell)
{
    const uint32_t f = (heads >> (16 * p)) & 0xFFFFu, cnt = f & 3u;
    const uint32_t g = cnt ? (f & ~3u) | 2u : 1u | ((uint32_t)cell << 2);
    return (heads & ~(0xFFFFu << (16 * p))) | (g << (16 * p));
}
__device__ __forceinline__ uint32_t heads_merged(uint32_t a, uint32_t b)
{
    uint32_t out = 0u;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint32_t fa = (a >> (16 * p)) & 0xFFFFu, fb = (b >> (16 * p)) & 0xFFFFu;
        const uint32_t cnt = min((fa & 3u) + (fb & 3u), 2u);
        out |= ((((fa & 3u) ? fa : fb) & ~3u) | cnt) << (16 * p);
    }
    return out;
}

// The lane's own board: word w of lane l at [w * 64 + l].
struct Board {
    uint32_t *words;                                                   // the lane's column: words + w * PO_LANES
    __device__ __forceinline__ uint32_t cell(int i) const { return (words[(i >> 4) * PO_LANES] >> (2 * (i & 15))) & 3u; }
};

// A safe move: the first-to-last directions UP, RIGHT, DOWN, LEFT whose target is EMPTY on the board as it stands (the
// heads' cells hold trails), candidates[mulhi(u, c)]; UP when there is none.
__device__ __forceinline__ int safe_move(const Board &bd, int S, int r, int c, uint32_t u)
{
    const int at = cell_index(S, r, c);
    uint32_t cand = 0u, cnt = 0u;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        int dr, dc;
        action_delta(a, dr, dc);
        if (bd.cell(at + dr * S + dc) == PO_EMPTY) {
            cand |= (uint32_t)a << (2u * cnt);
            ++cnt;
        }
    }
    return cnt ? (int)((cand >> (2u * __umulhi(u, cnt))) & 3u) : 0;
}
// The weighted safe move (file header): the same candidates, candidate a weighing byte k(a) of `weights`; the first one
// whose running sum of weights exceeds mulhi(u, sum).  Candidates that all weigh nothing weigh one each, which is
// safe_move's pick written as a running sum; UP when there is none.
__device__ __forceinline__ int safe_move_weighted(const Board &bd, int S, int r, int c, uint32_t u, uint32_t weights)
{
    const int at = cell_index(S, r, c);
    // the twelve cells around the head, one round trip: the four targets, the four diagonals (two targets' neighbour
    // each) and the four cells two steps on, which lie in the image when their target is strictly inside the border
    bool e[4], diag[4], far[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        int dr, dc, er, ec;
        action_delta(a, dr, dc);
        action_delta((a + 1) & 3, er, ec);
        const int t = at + dr * S + dc;
        const bool inside = on_board(S - 2, r + dr, c + dc);
        e[a] = bd.cell(t) == PO_EMPTY;
        diag[a] = bd.cell(t + er * S + ec) == PO_EMPTY;                // between directions a and a + 1
        far[a] = (bd.cell(inside ? t + dr * S + dc : t) == PO_EMPTY) && inside;
    }
    uint32_t w[4], cnt = 0u, total = 0u;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const uint32_t k = (uint32_t)diag[(a + 3) & 3] + (uint32_t)diag[a] + (uint32_t)far[a];
        w[a] = e[a] ? (weights >> (8u * k)) & 0xFFu : 0u;
        cnt += (uint32_t)e[a];
        total += w[a];
    }
    if (total == 0u) {
#pragma unroll
        for (int a = 0; a < 4; ++a) w[a] = (uint32_t)e[a];
        total = cnt;
    }
    const uint32_t x = __umulhi(u, total), s0 = w[0], s1 = s0 + w[1], s2 = s1 + w[2];
    return total ? (int)(x >= s0) + (int)(x >= s1) + (int)(x >= s2) : 0;
}
template <bool WEIGHTED>
__device__ __forceinline__ int drawn_move(const Board &bd, int S, int r, int c, uint32_t u, uint32_t weights)
{
    if constexpr (WEIGHTED) return safe_move_weighted(bd, S, r, c, u, weights);
    else return safe_move(bd, S, r, c, u);
}

// ---- the phases both kernels are made of ---------------------------------------------------------------------------------
// Boards in: `count` boards from board `first` on, through groups of GROUP lanes per board.  Lane (gb, sub) packs words
// sub, sub + GROUP, ... of boards gb, gb + 64 / GROUP, ... to dst[w * stride + b] and the group merges the heads it saw
// into info[b].  Every lane of the wave takes part, whatever `count` is.
template <int GROUP>
__device__ __forceinline__ void boards_in(const int8_t *__restrict__ codes, int64_t total, int G, int WORDS, int64_t first,
                                          int count, uint32_t *dst, int stride, uint32_t *info)
{
    const int sub = (int)threadIdx.x % GROUP, gb = (int)threadIdx.x / GROUP;
    for (int b0 = 0; b0 < count; b0 += PO_LANES / GROUP) {
        const int b = b0 + gb;
        const bool have_b = b < count;
        uint32_t heads = 0u;
        for (int w = sub; w < WORDS; w += GROUP) {
            if (!have_b) continue;
            uint32_t x[4];
            load16(codes, total, (first + b) * (int64_t)G + 16 * w, x);
            const int nvalid = min(16, G - 16 * w);                    // the bytes behind them are the next board's
            uint32_t word = 0u;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int v = i < nvalid ? (int)(int8_t)(x[i >> 2] >> (8 * (i & 3))) : -1;
                const uint32_t cls = v == 1 ? PO_EMPTY : (v == -2 || v == 10) ? PO_P1 : (v == -3 || v == -10) ? PO_P2 : PO_WALL;
                word |= cls << (2 * i);
                if (v == 10) heads = head_seen(heads, 0, 16 * w + i);
                if (v == -10) heads = head_seen(heads, 1, 16 * w + i);
            }
            dst[w * stride + b] = word;
        }
#pragma unroll
        for (int m = 1; m < GROUP; m <<= 1) heads = heads_merged(heads, (uint32_t)__shfl_xor((int)heads, m));
        if (sub == 0) info[b] = heads;
    }
}

// One playout as its lane carries it: the heads in board coordinates, the alive bits, how it ended (-1: not yet).
struct Playout {
    int r[2], c[2];
    uint32_t alive;
    int winner, steps;
    bool live;
};
// Playable: exactly one +10 and one -10, both strictly inside the border; a playout that is not never goes live.
__device__ __forceinline__ Playout playout_start(uint32_t heads, int S, bool have)
{
    Playout po;
    bool playable = have;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint32_t f = (heads >> (16 * p)) & 0xFFFFu;
        const int at = (int)(f >> 2), pr = at / S, pc = at - pr * S;
        playable = playable && (f & 3u) == 1u && pr >= 1 && pc >= 1 && pr <= S - 2 && pc <= S - 2;
        po.r[p] = pr - 1;
        po.c[p] = pc - 1;
    }
    po.alive = META_ALIVE0 | META_ALIVE1;
    po.winner = -1;
    po.steps = 0;
    po.live = playable;
    return po;
}
// Step t of the live playout `index`: `now` holds the two players' tape bytes (player 2's in bits 8..15).
// WEIGHTED (here and in the sliding step): a drawn move is safe_move_weighted under `weights`, else safe_move.
template <bool WEIGHTED>
__device__ __forceinline__ void playout_step(const Board &bd, int S, Playout &po, uint32_t now, uint32_t index, int t,
                                             uint32_t call_lo, uint32_t call_hi, uint32_t seed, uint32_t stream,
                                             uint32_t weights)
{
    int a[2] = {(int)(int8_t)now, (int)(int8_t)(now >> 8)};
    if ((a[0] | a[1]) < 0) {                                           // a negative byte: one Philox block serves both players
        uint32_t u[4];
        philox4x32_10(index, (uint32_t)t, call_lo, call_hi, seed, stream, u);
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (a[p] < 0) a[p] = drawn_move<WEIGHTED>(bd, S, po.r[p], po.c[p], u[p], weights);
    }
    // Game.step: both move, then each is judged on the cell it entered, player 2 after player 1's head is down
    int old[2], f[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        int dr, dc;
        action_delta(a[p] & 3, dr, dc);
        old[p] = cell_index(S, po.r[p], po.c[p]);
        po.r[p] += dr;
        po.c[p] += dc;
        f[p] = cell_index(S, po.r[p], po.c[p]);
    }
    uint32_t *w0 = bd.words + (f[0] >> 4) * PO_LANES, *w1 = bd.words + (f[1] >> 4) * PO_LANES;
    const uint32_t s0 = 2u * (uint32_t)(f[0] & 15), s1 = 2u * (uint32_t)(f[1] & 15);
    uint32_t x0 = *w0, x1 = *w1;
    uint32_t tf[2] = {(x0 >> s0) & 3u, (x1 >> s1) & 3u};
    plain_targets(old, f, tf, PO_P1, PO_P2, PO_P1_HEAD);
#pragma unroll
    for (int p = 0; p < 2; ++p) po.alive = collide(po.alive, p, S - 2, po.r[p], po.c[p], tf[p] == PO_EMPTY);
    // the new heads' cells take their owners' trails (what they are once the next step begins); a cell a player died
    // on is a head's cell of the last position, which the head byte covers
    x0 |= PO_P1 << s0;
    if (w1 == w0) x1 = x0;
    x1 |= PO_P2 << s1;
    *w0 = x0;
    *w1 = x1;
    po.steps = t + 1;
    int won = 0;
    if (settle(po.alive, po.r, po.c, won)) {
        po.winner = won;
        po.live = false;
    }
}

// The same step under the sliding rule (orc_step's order; game.py:158-214): player p's target n[p] is consumed when it is
// strictly inside the border and EMPTY as the board stands then, and with (double)u[p] <= rate[p] it takes p's trail and
// the head lands one cell further, on sl[p].  `taped`: u[] holds the caller's uniforms; else words 2 and 3 of the block.
template <bool WEIGHTED>
__device__ __forceinline__ void playout_step_slide(const Board &bd, int S, Playout &po, uint32_t now, const double rate[2],
                                                   bool taped, float u0, float u1, uint32_t index, int t, uint32_t call_lo,
                                                   uint32_t call_hi, uint32_t seed, uint32_t stream, uint32_t weights)
{
    int a[2] = {(int)(int8_t)now, (int)(int8_t)(now >> 8)};
    float u[2] = {u0, u1};
    if (!taped || (a[0] | a[1]) < 0) {                                 // one Philox block serves both players' move and slide
        uint32_t x[4];
        philox4x32_10(index, (uint32_t)t, call_lo, call_hi, seed, stream, x);
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (a[p] < 0) a[p] = drawn_move<WEIGHTED>(bd, S, po.r[p], po.c[p], x[p], weights);
        if (!taped) {                                                  // the env's conversion (tron_env.hip)
            u[0] = (float)(x[2] >> 8) * (1.0f / 16777216.0f);
            u[1] = (float)(x[3] >> 8) * (1.0f / 16777216.0f);
        }
    }
    // the four cells, read in one round trip: as the board stood before the step (the heads' cells hold trails)
    int dr[2], dc[2], n[2], sl[2];
    bool inb[2], en[2], es[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        action_delta(a[p] & 3, dr[p], dc[p]);
        inb[p] = on_board(S - 2, po.r[p] + dr[p], po.c[p] + dc[p]);
        n[p] = cell_index(S, po.r[p] + dr[p], po.c[p] + dc[p]);
        sl[p] = inb[p] ? n[p] + dr[p] * S + dc[p] : n[p];
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        en[p] = bd.cell(n[p]) == PO_EMPTY;
        es[p] = bd.cell(sl[p]) == PO_EMPTY;
    }
    // both move, player 2 on the board that holds player 1's slide tile of this step
    bool slid[2] = {false, false}, ef[2];
    int f[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const bool empty_now = en[p] && !(p == 1 && slid[0] && n[1] == n[0]);
        slid[p] = inb[p] && empty_now && (double)u[p] <= rate[p];
        f[p] = slid[p] ? sl[p] : n[p];
        ef[p] = slid[p] ? es[p] : empty_now;
        po.r[p] += slid[p] ? 2 * dr[p] : dr[p];
        po.c[p] += slid[p] ? 2 * dc[p] : dc[p];
    }
    // each is judged on the cell it entered, after both slide tiles, player 2 after player 1's head is down
    const bool ok[2] = {ef[0] && !(slid[1] && f[0] == n[1]), ef[1] && !(slid[0] && f[1] == n[0]) && f[1] != f[0]};
#pragma unroll
    for (int p = 0; p < 2; ++p) po.alive = collide(po.alive, p, S - 2, po.r[p], po.c[p], ok[p]);
    // the slide tiles and the new heads' cells take their owners' trails (see the file header)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const uint32_t trail = p == 0 ? PO_P1 : PO_P2;
        if (slid[p]) atomicOr(bd.words + (n[p] >> 4) * PO_LANES, trail << (2u * (uint32_t)(n[p] & 15)));
        atomicOr(bd.words + (f[p] >> 4) * PO_LANES, trail << (2u * (uint32_t)(f[p] & 15)));
    }
    po.steps = t + 1;
    int won = 0;
    if (settle(po.alive, po.r, po.c, won)) {
        po.winner = won;
        po.live = false;
    }
}

// SLIDE: the sliding rule under `rates` f64[n][2] and `uniforms` f32[k_steps][n][2] or nullptr (k_playout_slide); without it
// the two are not looked at (k_playout).  WEIGHTED: drawn moves are weighted by `weights`, byte k the weight of room k
// (k_playout_weighted, k_playout_slide_weighted); without it `weights` is not looked at.
template <bool SLIDE, bool WEIGHTED>
__global__ __launch_bounds__(PO_LANES) void k_playout_t(const int8_t *__restrict__ codes, int64_t n, int S, int k_steps,
                                                        const int8_t *__restrict__ actions, uint32_t seed, uint32_t stream,
                                                        uint32_t call_lo, uint32_t call_hi, int32_t *__restrict__ out_steps,
                                                        int8_t *__restrict__ out_winner, int8_t *__restrict__ out_codes,
                                                        const double *__restrict__ rates, const float *__restrict__ uniforms,
                                                        uint32_t weights)
{
    extern __shared__ uint32_t po_lds[];
    const int lane = threadIdx.x, G = S * S, WORDS = (G + 15) >> 4;
    uint32_t *info = po_lds + WORDS * PO_LANES;                        // [64] one word per board, between the phases
    const int64_t first = (int64_t)blockIdx.x * PO_LANES, idx = first + lane, total = n * (int64_t)G;
    const int sub = lane % PO_GROUP, gb = lane / PO_GROUP;
    const bool have = idx < n;

    boards_in<PO_GROUP>(codes, total, G, WORDS, first, (int)min((int64_t)PO_LANES, n - first), po_lds, PO_LANES, info);
    __syncthreads();
    const Board bd{po_lds + lane};
    Playout po = playout_start(have ? info[lane] : 0u, S, have);
    const bool playable = po.live;

    // ---- the steps.  A lane that is finished or rejected idles; the wave leaves when its last lane is done
    const int8_t *tape = actions ? actions + 2 * idx : nullptr;        // row t: tape + t * 2n
    auto tape_row = [&](int t) {
        uint16_t v;
        __builtin_memcpy(&v, tape + (int64_t)t * 2 * n, 2);
        return (uint32_t)v;
    };
    uint32_t ahead = (tape && po.live && k_steps > 0) ? tape_row(0) : 0xFFFFu;
    if constexpr (!SLIDE) {
        for (int t = 0; t < k_steps; ++t) {
            if (!__ballot(po.live)) break;
            const uint32_t now = ahead;
            if (tape && po.live && t + 1 < k_steps) ahead = tape_row(t + 1);   // one step ahead of its use
            if (!po.live) continue;
            playout_step<WEIGHTED>(bd, S, po, now, (uint32_t)idx, t, call_lo, call_hi, seed, stream, weights);
        }
    } else {
        const double rate[2] = {have ? rates[2 * idx] : -1.0, have ? rates[2 * idx + 1] : -1.0};
        const float *utape = uniforms ? uniforms + 2 * idx : nullptr;  // row t: utape + t * 2n, read as the action tape is
        auto utape_row = [&](int t) { return make_float2(utape[(int64_t)t * 2 * n], utape[(int64_t)t * 2 * n + 1]); };
        float2 uahead = (utape && po.live && k_steps > 0) ? utape_row(0) : make_float2(0.0f, 0.0f);
        for (int t = 0; t < k_steps; ++t) {
            if (!__ballot(po.live)) break;
            const uint32_t now = ahead;
            const float2 unow = uahead;
            if (tape && po.live && t + 1 < k_steps) ahead = tape_row(t + 1);
            if (utape && po.live && t + 1 < k_steps) uahead = utape_row(t + 1);
            if (!po.live) continue;
            playout_step_slide<WEIGHTED>(bd, S, po, now, rate, utape != nullptr, unow.x, unow.y, (uint32_t)idx, t, call_lo,
                                         call_hi, seed, stream, weights);
        }
    }
    if (have) {
        if (out_steps) out_steps[idx] = playable ? po.steps : 0;
        if (out_winner) out_winner[idx] = (int8_t)(playable ? po.winner : -2);
    }
    if (!out_codes) return;

    // ---- boards out: the last position's cells from LDS with the two head bytes on top, player 2's last (game.py:205-214);
    // a rejected board, and every board of a call of no steps, is its input copied
    info[lane] = (playable && k_steps > 0) ? (uint32_t)cell_index(S, po.r[0], po.c[0]) | ((uint32_t)cell_index(S, po.r[1], po.c[1]) << 11)
                                           : PO_COPY;
    __syncthreads();
    constexpr uint32_t CODE_OF = pack4(1, -2, -3, -1);                 // PO_EMPTY, PO_P1, PO_P2, PO_WALL as player 1 sees them
    for (int b0 = 0; b0 < PO_LANES; b0 += PO_BOARDS) {
        const int b = b0 + gb;
        if (first + b >= n) continue;
        const uint32_t inf = info[b];
        for (int w = sub; w < WORDS; w += PO_GROUP) {
            const int64_t at = (first + b) * (int64_t)G + 16 * w;
            uint32_t x[4];
            if (inf & PO_COPY) {
                load16(codes, total, at, x);
            } else {
                const uint32_t word = po_lds[w * PO_LANES + b];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t q = word >> (8 * j);                // four cells' classes, one per selector byte
                    x[j] = __builtin_amdgcn_perm(0u, CODE_OF, (q & 3u) | ((q & 0xCu) << 6) | ((q & 0x30u) << 12) | ((q & 0xC0u) << 18));
                }
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int h = (int)((inf >> (11 * p)) & 0x7FFu);
                    if ((h >> 4) != w) continue;
                    const uint32_t sh = 8u * (uint32_t)(h & 3), byte = p == 0 ? 10u : (uint32_t)(uint8_t)-10;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (((h & 15) >> 2) == j) x[j] = (x[j] & ~(0xFFu << sh)) | (byte << sh);
                }
            }
            store16(out_codes + at, min(16, G - 16 * w), x);
        }
    }
}

constexpr auto k_playout = k_playout_t<false, false>, k_playout_slide = k_playout_t<true, false>;
constexpr auto k_playout_weighted = k_playout_t<false, true>, k_playout_slide_weighted = k_playout_t<true, true>;

// ---- Monte-Carlo move values (tron_playout_values) --------------------------------------------------------------------------
//   k_playout_values  k_playout's lanes and step loop over launch indices q = ((board * 16 + a1 * 4 + a2) * copies + j):
//               the board and the first move come from q, no tape and no copied board exist.  A wave's 64 consecutive
//               indices meet at most PV_SLOTS boards (16 * copies >= 16 indices per board: 5 at the most).  Each is read
//               from global memory once, by a group of 16 lanes, classified once into a staging table [word][slot], and
//               copied from there into the column of every lane that plays it (a read of at most 5 addresses on 5
//               different banks, a write to the lane's own bank).  The endings are summed in LDS, [slot][move][4 classes
//               and the steps], and each non-zero sum goes out as one global integer add: sums of integers, so the order
//               of arrival changes nothing.
//   k_values_pick     one lane per board, after the tallies: the maximin of m = wins of 1 - wins of 2 for either player.
constexpr int PV_GROUP = 16;                       // lanes that share a board while k_playout_values loads it
constexpr int PV_SLOTS = 8;                        // room for the boards of one wave (two rounds of 64 / PV_GROUP)
constexpr int PV_ROW = 5;                          // one (board, first move): draws, wins of 1, wins of 2, unfinished, steps
constexpr int PV_TALLY = PV_SLOTS * 16 * PV_ROW;

// SLIDE: the sliding rule, board i's row of `rates` f64[n][2] for all its playouts (k_playout_values_slide).  WEIGHTED: as
// in k_playout_t (k_playout_values_weighted, k_playout_values_slide_weighted).
template <bool SLIDE, bool WEIGHTED>
__global__ __launch_bounds__(PO_LANES) void k_playout_values_t(const int8_t *__restrict__ codes, int64_t n, int S, int k_steps,
                                                               uint32_t copies, uint32_t seed, uint32_t stream,
                                                               uint32_t call_lo, uint32_t call_hi,
                                                               int32_t *__restrict__ out_counts,
                                                               int32_t *__restrict__ out_steps,
                                                               const double *__restrict__ rates, uint32_t weights)
{
    extern __shared__ uint32_t po_lds[];
    const int lane = threadIdx.x, G = S * S, WORDS = (G + 15) >> 4;
    uint32_t *info = po_lds + WORDS * PO_LANES;                        // [PV_SLOTS] the heads of the wave's boards
    uint32_t *stage = info + PO_LANES;                                 // [WORDS][PV_SLOTS] the wave's boards, packed
    int *tally = reinterpret_cast<int *>(stage + WORDS * PV_SLOTS);    // [PV_SLOTS][16][PV_ROW]
    const uint32_t per = 16u * copies, nq = (uint32_t)n * per;          // n * 16 * copies < 2^31 (checked by the entry)
    const uint32_t first = blockIdx.x * (uint32_t)PO_LANES, q = first + (uint32_t)lane;
    const uint32_t b_lo = first / per, b_hi = min(first + (uint32_t)(PO_LANES - 1), nq - 1u) / per;
    const int nb = (int)(b_hi - b_lo) + 1;                             // <= 63 / 16 + 2 = 5
    const bool have = q < nq;
    const int lb = have ? (int)(q / per - b_lo) : 0, move = (int)((q / copies) & 15u);

    for (int e = lane; e < PV_TALLY; e += PO_LANES) tally[e] = 0;
    boards_in<PV_GROUP>(codes, n * (int64_t)G, G, WORDS, (int64_t)b_lo, nb, stage, PV_SLOTS, info);
    __syncthreads();
    const Board bd{po_lds + lane};
    if (have)
        for (int w = 0; w < WORDS; ++w) bd.words[w * PO_LANES] = stage[w * PV_SLOTS + lb];
    Playout po = playout_start(info[lb], S, have);
    const bool playable = po.live;

    // ---- the steps: the first from the index, every later one a safe draw for both
    double rate[2] = {-1.0, -1.0};
    if constexpr (SLIDE) {
        if (have) {
            rate[0] = rates[2 * (int64_t)(q / per)];
            rate[1] = rates[2 * (int64_t)(q / per) + 1];
        }
    }
    for (int t = 0; t < k_steps; ++t) {
        if (!__ballot(po.live)) break;
        if (!po.live) continue;
        const uint32_t now = t ? 0xFFFFu : (uint32_t)(move >> 2) | ((uint32_t)(move & 3) << 8);
        if constexpr (SLIDE)
            playout_step_slide<WEIGHTED>(bd, S, po, now, rate, false, 0.0f, 0.0f, q, t, call_lo, call_hi, seed, stream, weights);
        else
            playout_step<WEIGHTED>(bd, S, po, now, q, t, call_lo, call_hi, seed, stream, weights);
    }

    // ---- the tallies: winner -1, 0, 1, 2 is class 3, 0, 1, 2
    if (playable) {
        int *row = tally + (lb * 16 + move) * PV_ROW;
        atomicAdd(row + (po.winner & 3), 1);
        if (po.steps) atomicAdd(row + 4, po.steps);
    }
    __syncthreads();
    for (int e = lane; e < nb * 16 * PV_ROW; e += PO_LANES) {
        const int v = tally[e];
        if (!v) continue;
        const int64_t at = (int64_t)b_lo * 16 + e / PV_ROW;            // (board, first move)
        const int c = e % PV_ROW;
        if (c < 4) {
            if (out_counts) atomicAdd(out_counts + at * 4 + c, v);
        } else if (out_steps) {
            atomicAdd(out_steps + at, v);
        }
    }
}

constexpr auto k_playout_values = k_playout_values_t<false, false>, k_playout_values_slide = k_playout_values_t<true, false>;
constexpr auto k_playout_values_weighted = k_playout_values_t<false, true>,
               k_playout_values_slide_weighted = k_playout_values_t<true, true>;

__global__ __launch_bounds__(256) void k_values_pick(const int32_t *__restrict__ counts, int64_t n, int8_t *__restrict__ out_actions)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t *c = counts + i * 64;
    int m[4][4];
#pragma unroll
    for (int a1 = 0; a1 < 4; ++a1)
#pragma unroll
        for (int a2 = 0; a2 < 4; ++a2) m[a1][a2] = c[(a1 * 4 + a2) * 4 + 1] - c[(a1 * 4 + a2) * 4 + 2];
    if (c[0] + c[1] + c[2] + c[3] == 0) {                              // a playable board's rows sum to copies >= 1
        out_actions[2 * i] = out_actions[2 * i + 1] = (int8_t)-1;
        return;
    }
    int best[2] = {0, 0}, best_v[2] = {0, 0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        int v[2] = {m[a][0], -m[0][a]};
#pragma unroll
        for (int o = 1; o < 4; ++o) {
            v[0] = min(v[0], m[a][o]);
            v[1] = min(v[1], -m[o][a]);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)
            if (a == 0 || v[p] > best_v[p]) {
                best[p] = a;
                best_v[p] = v[p];
            }
    }
    out_actions[2 * i] = (int8_t)best[0];
    out_actions[2 * i + 1] = (int8_t)best[1];
}

}  // namespace

// The entries differ in the kernel alone: rates == nullptr launches a mode-None kernel, weights == nullptr one of the
// uniform draw (whose `weights` argument is not looked at).
static int launch_playout(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, const int8_t *actions, const double *rates,
                          const float *uniforms, const uint32_t *weights, uint32_t seed, uint32_t stream_id, uint64_t call,
                          int32_t *out_steps, int8_t *out_winner, int8_t *out_codes, void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || k_steps < 0 || (!codes && n > 0) || (out_codes && out_codes == codes)) return TRON_ERR_BAD_ARG;
    if (side < 6 || side > 34) return TRON_ERR_UNSUPPORTED;
    if (n == 0) return TRON_OK;
    const int words = (side * side + 15) >> 4;
    const size_t smem = (size_t)(words + 1) * PO_LANES * sizeof(uint32_t);     // 18 944 bytes at side 34: no LDS opt-in
    const dim3 grid((unsigned)((n + PO_LANES - 1) / PO_LANES));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const auto kernel = weights ? (rates ? k_playout_slide_weighted : k_playout_weighted) : (rates ? k_playout_slide : k_playout);
    hipLaunchKernelGGL(kernel, grid, dim3(PO_LANES), smem, st, codes, n, side, k_steps, actions, seed, stream_id, (uint32_t)call,
                       (uint32_t)(call >> 32), out_steps, out_winner, out_codes, rates, rates ? uniforms : nullptr,
                       weights ? *weights : 0u);
    return hipGetLastError() == hipSuccess ? TRON_OK : TRON_ERR_LAUNCH;
}

extern "C" int tron_playout_codes(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, const int8_t *actions,
                                  uint32_t seed, uint32_t stream_id, uint64_t call, int32_t *out_steps, int8_t *out_winner,
                                  int8_t *out_codes, void *stream)
{
    return launch_playout(codes, n, side, k_steps, actions, nullptr, nullptr, nullptr, seed, stream_id, call, out_steps,
                          out_winner, out_codes, stream);
}

extern "C" int tron_playout_slide_codes(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, const int8_t *actions,
                                        const double *rates, const float *uniforms, uint32_t seed, uint32_t stream_id,
                                        uint64_t call, int32_t *out_steps, int8_t *out_winner, int8_t *out_codes, void *stream)
{
    if (!rates && n > 0) return TRON_ERR_BAD_ARG;
    return launch_playout(codes, n, side, k_steps, actions, rates, uniforms, nullptr, seed, stream_id, call, out_steps,
                          out_winner, out_codes, stream);
}

extern "C" int tron_playout_weighted_codes(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, const int8_t *actions,
                                           const double *rates, const float *uniforms, uint32_t weights, uint32_t seed,
                                           uint32_t stream_id, uint64_t call, int32_t *out_steps, int8_t *out_winner,
                                           int8_t *out_codes, void *stream)
{
    if (uniforms && !rates) return TRON_ERR_BAD_ARG;
    return launch_playout(codes, n, side, k_steps, actions, rates, uniforms, &weights, seed, stream_id, call, out_steps,
                          out_winner, out_codes, stream);
}

static int launch_values(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, int32_t copies, const double *rates,
                         const uint32_t *weights, uint32_t seed, uint32_t stream_id, uint64_t call, int32_t *out_counts,
                         int32_t *out_steps, int8_t *out_actions, void *stream)
{
    constexpr int64_t LIMIT = (int64_t)1 << 31;                        // the Philox index and the sums are 32 bits
    if (n < 0 || k_steps < 0 || copies < 1 || (!codes && n > 0)) return TRON_ERR_BAD_ARG;
    if (n >= LIMIT || n * 16 >= LIMIT || n * 16 * copies >= LIMIT || (int64_t)copies * k_steps >= LIMIT) return TRON_ERR_BAD_ARG;
    if (side < 6 || side > 34) return TRON_ERR_UNSUPPORTED;
    if (n == 0) return TRON_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the actions are read off the counts: without a buffer of the caller's they are tallied in one that lives for this call
    int32_t *counts = out_counts;
    const size_t counts_bytes = (size_t)n * 64 * sizeof(int32_t);
    if (!counts && out_actions && hipMallocAsync(reinterpret_cast<void **>(&counts), counts_bytes, st) != hipSuccess) {
        (void)hipGetLastError();
        return TRON_ERR_LAUNCH;
    }
    bool ok = (!counts || hipMemsetAsync(counts, 0, counts_bytes, st) == hipSuccess) &&
              (!out_steps || hipMemsetAsync(out_steps, 0, (size_t)n * 16 * sizeof(int32_t), st) == hipSuccess);
    if (ok && (counts || out_steps)) {
        const int words = (side * side + 15) >> 4;
        const size_t smem = ((size_t)(words + 1) * PO_LANES + (size_t)words * PV_SLOTS + PV_TALLY) * sizeof(uint32_t);   // 23 840 bytes at side 34
        const int64_t nq = n * 16 * copies;
        const dim3 grid((unsigned)((nq + PO_LANES - 1) / PO_LANES));
        const auto kernel = weights ? (rates ? k_playout_values_slide_weighted : k_playout_values_weighted)
                                    : (rates ? k_playout_values_slide : k_playout_values);
        hipLaunchKernelGGL(kernel, grid, dim3(PO_LANES), smem, st, codes, n, side, k_steps, (uint32_t)copies, seed, stream_id,
                           (uint32_t)call, (uint32_t)(call >> 32), counts, out_steps, rates, weights ? *weights : 0u);
        if (out_actions)
            hipLaunchKernelGGL(k_values_pick, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, counts, n, out_actions);
    }
    ok = hipGetLastError() == hipSuccess && ok;
    if (counts != out_counts) ok = hipFreeAsync(counts, st) == hipSuccess && ok;
    return ok ? TRON_OK : TRON_ERR_LAUNCH;
}

extern "C" int tron_playout_values(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, int32_t copies, uint32_t seed,
                                   uint32_t stream_id, uint64_t call, int32_t *out_counts, int32_t *out_steps,
                                   int8_t *out_actions, void *stream)
{
    return launch_values(codes, n, side, k_steps, copies, nullptr, nullptr, seed, stream_id, call, out_counts, out_steps, out_actions,
                         stream);
}

extern "C" int tron_playout_slide_values(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, int32_t copies,
                                         const double *rates, uint32_t seed, uint32_t stream_id, uint64_t call,
                                         int32_t *out_counts, int32_t *out_steps, int8_t *out_actions, void *stream)
{
    if (!rates && n > 0) return TRON_ERR_BAD_ARG;
    return launch_values(codes, n, side, k_steps, copies, rates, nullptr, seed, stream_id, call, out_counts, out_steps, out_actions,
                         stream);
}

extern "C" int tron_playout_weighted_values(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, int32_t copies,
                                            const double *rates, uint32_t weights, uint32_t seed, uint32_t stream_id,
                                            uint64_t call, int32_t *out_counts, int32_t *out_steps, int8_t *out_actions,
                                            void *stream)
{
    return launch_values(codes, n, side, k_steps, copies, rates, &weights, seed, stream_id, call, out_counts, out_steps,
                         out_actions, stream);
}

// k_values_pick alone, on counts the caller tallied itself (tron.vec.playout_values(judge=...)).
extern "C" int tron_values_pick(const int32_t *counts, int64_t n, int8_t *out_actions, void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || ((!counts || !out_actions) && n > 0)) return TRON_ERR_BAD_ARG;
    if (n == 0) return TRON_OK;
    hipLaunchKernelGGL(k_values_pick, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), counts,
                       n, out_actions);
    return hipGetLastError() == hipSuccess ? TRON_OK : TRON_ERR_LAUNCH;
}
