// gfx950 kernels + C ABI for the vectorised TRON env (include/tron_hip.h).
//
// Data layout.  Everything is env-major: grid[N][G] int8, obs[N][2][...],
// one uint4 of hot state words per env.  A 256-thread workgroup owns a tile of E consecutive
// envs, cut into per-env 16-byte chunks (CPE = ceil(G/16) per env, the last one possibly
// short) so a chunk never spans envs; chunk i of the tile sits in LDS slot i.
//
// k_tile, one launch = one Game.step for every env + both players' observations:
//   1  all threads: chunk loads HBM -> registers -> LDS (6 loads in flight per thread).
//      In the shadow of that load wave 0, ONE ENV PER LANE, does all the random-number
//      work the step can need: the Philox block for actions / slide uniforms and,
//      speculatively, the start of the game after next (both need only the counters);
//   2  barrier; wave 0 plays the move against the LDS tile — reads its 2-4 cells, writes
//      its <=6 cells, marks their chunks in an LDS bitmask — and leaves its results
//      (new state words, done/winner/reward, restart words) in LDS records.  It issues
//      no global store: under store back-pressure each one would stall the lone wave;
//   3  barrier; waves 1-3 write the records out (one array each), then ALL threads
//      stream: LDS chunk (or the fresh-board template + heads for a restarted env) ->
//      v_perm byte LUT -> two coalesced 16-byte stores, plus a predicated write-back of
//      the grid chunk when it is dirty or its env restarted.
// HBM sees one coalesced read of the grid, one coalesced write of both observation
// planes, ~4 dirty 16-byte chunks per env, and ~100 bytes of state/outputs per env.
// A lone wave retires about one instruction per five cycles, so the serial section
// between the barriers is LDS-only and ~200 instructions; everything heavier is off it.
//
// Kernels in this file:
//   k_tile / tile_step      board-owning layout (grid[N][G] + caller's obs): every mode, format, side
//   k_obs / obs_tile        observation-is-state (mode None, int8 codes, even side): the caller's
//                           attached obs buffer is the env state; read G, write 2G per env-step
//   k_obs_roll, k_tile_roll tron_rollout_random: up to ROLL_LAUNCH_CAP (k_obs_roll) / TRON_ROLLOUT_CHUNK steps in ONE launch.  k_obs_roll (roll_resident):
//                           one lane per env and a game wave that owns its envs for the whole launch, with a helper wave
//                           beside it on its SIMD that draws every Philox word of the launch into LDS rings (one
//                           workgroup barrier per block of ROLL_R steps, none inside a block: roll_helper),
//                           boards in LDS at 4 bits per cell (the whole batch resident in one round), memory read in the
//                           prologue only and WRITTEN IN THE EPILOGUE ONLY: a step touches LDS and registers, and the
//                           launch's end stores the chunks its steps touched (both planes from the packed board, the
//                           player-2 one swapped in nibble space); a restart rebuilds its board in LDS and takes its next
//                           game's starts from the helper's ring (make_game_starts; the weights and the degree are drawn
//                           in the epilogue).  The per-step forms (k_obs, TRON_ROLLOUT_PER_STEP,
//                           the kernels below) have every step's planes in memory.  k_tile_roll, k_obs_roll_walk
//                           (boards of more than 64 chunks, TRON_ROLL_GRID) and k_obs_roll_slide: the per-tile step
//                           (tile_step / obs_tile), each workgroup stepping its own tiles
//   k_obs_roll_tape         tron_rollout_actions: k_obs_roll's launch (roll_resident<true>) whose helper wave copies the
//                           action bytes from the caller's tape into the ring instead of drawing them
//   k_obs_roll_tape_rec     tron_rollout_actions_records: k_obs_roll_tape (roll_resident<true, true>) whose game waves also
//                           store every step's done / winner / reward into the caller's step-major record tapes
//   k_inc                   TRON_STEP_INCREMENTAL: writes only the touched cells + restarted boards
//   k_reset, k_obs_reset, k_obs_to_grid, k_obs_planes, k_get_state, k_encode_codes, k_pop_up, ...
//                           resets, read-back and stateless encodes
//
// Where the rule lives.  Game.next_frame + Game.step (game.py:149-277) as register arithmetic — action table, what a
// player hits, collisions, done / winner, rewards, the st4 words, the restart word — is written once, in tron_device.hpp
// ("the rule"); the slide decision (temper_threshold, slides) and the per-tile kernels' records (move_records) are below.
// A kernel's move is those helpers plus its own cell reads and writes:
//   k_tile, k_tile_roll                       lane_move<BoardCells>  six-cell sliding move on Tile bytes in LDS, dirty-chunk bits
//   k_obs_slide, k_obs_roll_slide             lane_move<CodeCells>   the same body on player-1 code bytes, slide marks
//   k_obs, k_obs_roll_walk                    lane_move_codes        mode None: two reads, four writes of code bytes in LDS
//   k_inc                                     inline in the kernel   lane_move_codes' steps on code bytes in global memory
//   k_obs_roll, k_obs_roll_tape(_rec)         inline in roll_resident  the same steps on 4-bit codes in LDS, with the chunk masks
#include "tron_device.hpp"
#include "tron_launch.hpp"
#include "tron_minimax.hpp"
#include "../../include/tron_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>
#include <new>
#include <type_traits>
#include <type_traits>

using namespace tron;

namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;
constexpr int DK = 6;            // 16-byte loads per thread in flight per batch

struct StepOut {
    int8_t *done;
    int8_t *winner;
    float *reward;
    unsigned long long *totals;
};

// Diagnostic build only (-DTRON_STAMPS): out.totals is then a stamp buffer of s_memrealtime ticks (100 MHz) for wave 0
// and wave 1 of every workgroup; never enabled in the shipped library.  Two layouts: [blocks][2][8], one block of slots per
// launch (STAMP: the per-tile kernels), and [blocks][2][TRON_ROLLOUT_CHUNK + 1][4], one block per step (ROLL_STAMP) and a
// last one for the launch (ROLL_STAMP_LAUNCH: 0 kernel entry, 1 step loop left, 2 plane stores issued, 3 kernel end), both
// of roll_resident, read by scripts/roll_stamps.py.  blocks is the launch's grid: ceil(N / 64) when k_obs_roll runs one
// wave per workgroup (roll_waves), where only wave 0's half is written.
// Behind that region, at ceil(N / 64) * 2 * (TRON_ROLLOUT_CHUNK + 1) * 4 whatever the grid, the helpers of the stamped game
// waves have their own: [blocks][2][ROLL_HSTAMPS] (ROLL_HSTAMP: 0 kernel entry, 1 prologue draws done, 2 arrival at P, 3
// departure from P, 2 + 2 b / 3 + 2 b arrival at / departure from B_b; the last slot but one is the end of the hand-off
// pass, which begins at the departure from B_(nb-1), or from P in a launch of one block; behind a handed entry slot 1 is
// "the handed words are in the rings"; the last slot is the GAME wave's arrival at P, which its own layout has no place for).
// A launch may be longer than TRON_ROLLOUT_CHUNK steps (ROLL_LAUNCH_CAP) and the regions are not: the first
// TRON_ROLLOUT_CHUNK steps and the barriers in front of the first TRON_ROLLOUT_CHUNK / 8 blocks are stamped (ROLL_STAMP,
// ROLL_HSTAMP_BLOCK: the step or block is tested against the region before the store), the later ones are not, and the
// launch-level slots are the whole launch's.
#ifdef TRON_STAMPS
constexpr int ROLL_HSTAMPS = 4 + 2 * (TRON_ROLLOUT_CHUNK / 8);
#define ROLL_HSTAMP(slot)                                                                         \
    do {                                                                                          \
        if (out.totals && lane == 0 && wave < (gw > 1 ? 2 : 1))                                   \
            out.totals[((size_t)((P.N + 63) / 64) * 2 * (TRON_ROLLOUT_CHUNK + 1)) * 4 + ((size_t)blockIdx.x * 2 + wave) * ROLL_HSTAMPS + (slot)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define STAMP(slot)                                                                               \
    do {                                                                                          \
        if (out.totals && (tid == 0 || tid == 64))                                                \
            out.totals[((size_t)blockIdx.x * 2 + (tid >> 6)) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define ROLL_HSTAMP_BLOCK(b, k)                                                                   \
    do {                                                                                          \
        if ((b) < TRON_ROLLOUT_CHUNK / 8) ROLL_HSTAMP(2 + 2 * (b) + (k));                         \
    } while (0)
#define ROLL_STAMP(slot)                                                                          \
    do {                                                                                          \
        if (out.totals && s < TRON_ROLLOUT_CHUNK && (tid == 0 || (tid == 64 && gw > 1)))                    \
            out.totals[(((size_t)blockIdx.x * 2 + (tid >> 6)) * (TRON_ROLLOUT_CHUNK + 1) + s) * 4 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define ROLL_STAMP_LAUNCH(slot)                                                                   \
    do {                                                                                          \
        if (out.totals && (tid == 0 || (tid == 64 && gw > 1)))                                              \
            out.totals[(((size_t)blockIdx.x * 2 + (tid >> 6)) * (TRON_ROLLOUT_CHUNK + 1) + TRON_ROLLOUT_CHUNK) * 4 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define STAMP(slot) do { } while (0)
#define ROLL_STAMP(slot) do { } while (0)
#define ROLL_STAMP_LAUNCH(slot) do { } while (0)
#define ROLL_HSTAMP(slot) do { } while (0)
#define ROLL_HSTAMP_BLOCK(b, k) do { } while (0)
#endif

struct __attribute__((packed, aligned(4))) U4A4 {   // 16 bytes at 4-byte alignment
    uint32_t x, y, z, w;
};

// ---- global access of one chunk: 16-byte ops when G % 4 == 0, bytes otherwise ----
template <bool ALIGNED>
__device__ __forceinline__ uint4 load_chunk(const int8_t *p)
{
    if (ALIGNED) {
        const U4A4 v = *reinterpret_cast<const U4A4 *>(p);          // allocation is padded: over-read is safe
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 2] |= (uint32_t)(uint8_t)p[j] << ((j & 3) * 8);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
template <bool ALIGNED>
__device__ __forceinline__ void store_chunk(int8_t *p, int nb, const uint32_t w[4])
{
    if (ALIGNED) {
        if (nb == 16) {
            *reinterpret_cast<U4A4 *>(p) = U4A4{w[0], w[1], w[2], w[3]};
        } else {
            for (int j = 0; j < (nb >> 2); ++j) reinterpret_cast<uint32_t *>(p)[j] = w[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < nb) p[j] = (int8_t)(w[j >> 2] >> ((j & 3) * 8));
    }
}

// one chunk (nb valid cells of one env starting at cell c) -> both players' observations
template <int FMT, bool ALIGNED>
__device__ __forceinline__ void store_chunk_obs(void *__restrict__ obs, size_t env, int G, uint32_t c, int nb,
                                                const uint32_t w[4], float p4)
{
    if (FMT == TRON_OBS_CODES_I8) {
        int8_t *o1 = reinterpret_cast<int8_t *>(obs) + env * 2u * G + c;
        const uint32_t c1[4] = {codes4(w[0], false), codes4(w[1], false), codes4(w[2], false), codes4(w[3], false)};
        const uint32_t c2[4] = {codes4(w[0], true), codes4(w[1], true), codes4(w[2], true), codes4(w[3], true)};
        store_chunk<ALIGNED>(o1, nb, c1);
        store_chunk<ALIGNED>(o1 + G, nb, c2);
    } else if (FMT == TRON_OBS_PLANES3_F32 || FMT == TRON_OBS_PLANES4_F32) {
        constexpr int CH = (FMT == TRON_OBS_PLANES3_F32) ? 3 : 4;
        float *ob = reinterpret_cast<float *>(obs) + env * 2u * CH * G + c;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                float *dst = ob + (size_t)(p * CH + ch) * G;
                const uint32_t bits = (ch < 3) ? plane_bits(ch, p != 0) : 0u;
                if (ALIGNED) {                                       // G % 4 == 0: 16-byte aligned rows of 4 cells
                    for (int j = 0; j < (nb >> 2); ++j)
                        reinterpret_cast<float4 *>(dst)[j] =
                            (ch == 3) ? make_float4(p4, p4, p4, p4)
                                      : make_float4(plane_val(bits, w[j]), plane_val(bits, w[j] >> 8),
                                                    plane_val(bits, w[j] >> 16), plane_val(bits, w[j] >> 24));
                } else {
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (j < nb) dst[j] = (ch == 3) ? p4 : plane_val(bits, w[j >> 2] >> ((j & 3) * 8));
                }
            }
        }
    }
}

// state words of one env, loaded ahead of the tile
// chunk index -> env within the tile: i / cpe by multiplication with ceil(2^32 / cpe); that constant
// does not fit 32 bits for cpe == 1 (boards of at most 16 cells), where the quotient is i itself
__device__ __forceinline__ uint32_t chunk_env(uint32_t i, uint32_t cpe, uint32_t cpe_magic)
{
    return cpe == 1u ? i : __umulhi(i, cpe_magic);
}

// Game.get_rate (game.py:100-102) as a table: "temper" mode compares a float32 uniform with the float64 rate of
// (degree, weight); for every (degree in [-30, 30], weight in [40, 101]) — the ranges Game.__init__ draws from
// (game.py:83,87) — the table holds the largest float32 t with (double)t <= rate, so `u <= t` decides exactly what
// `(double)u <= rate` decides, without two float64 divisions per player in the one-env-per-lane section of the step.
// Filled once per process by tron_create (host arithmetic, same operation order); values assigned from outside the
// ranges (tron_set_weight_degree) take the float64 path.
constexpr int RATE_DEG = 61, RATE_W = 62;
__device__ float g_rate_thr[RATE_DEG * RATE_W];

struct EnvRegs {
    uint32_t pos, meta, eplen, tick;           // st4
    uint32_t envp, episode, nstart, nenvp;     // rs4
    uint32_t act;                              // a0 | a1 << 8 when the caller supplies actions
    float u0, u1;                              // slide uniforms when the caller supplies them
    double slide;
};

// ------------------------------------------------------------------ the rule --
// Game.next_frame + Game.step (game.py:149-277).  Its register arithmetic is written once, in tron_device.hpp ("the
// rule"): action_delta, plain_targets, collide, settle, step_rewards, pack_meta / stepped_st4 / restarted_st4,
// restart_word.  Here: the slide decision (it reads g_rate_thr), the records of the per-tile kernels, and the sliding move.

// "temper": player p's slide threshold from the table (ok: its degree and weight are inside the table's ranges).  The
// move asks for both players' before anything else, so that they arrive under the cell reads.
__device__ __forceinline__ void temper_threshold(uint32_t envp, int p, float &thr, bool &ok)
{
    const uint32_t di = (uint32_t)((int)(int8_t)(envp >> 16) + 30);
    const uint32_t wi = ((envp >> (8 * p)) & 0xFFu) - 40u;
    ok = di < (uint32_t)RATE_DEG && wi < (uint32_t)RATE_W;
    thr = g_rate_thr[ok ? di * RATE_W + wi : 0u];
}
// game.py:169: random.random() <= rate — "ice": the env's slide rate; "temper": the table, or float64 get_rate outside it
__device__ __forceinline__ bool slides(const Params &P, const EnvRegs &R, int p, float u, float thr, bool ok)
{
    if (P.mode == TRON_MODE_ICE) return (double)u <= R.slide;
    if (ok) return u <= thr;
    return (double)u <= get_rate((int)(int8_t)(R.envp >> 16), (int)((R.envp >> (8 * p)) & 0xFFu));
}

// Result records left in LDS by the move of the per-tile kernels (tile_step, obs_tile), read by waves 1-3 and by the
// stream: rec_st = the new st4; rec_out = {RES_* flags | winner << 4, reward1, reward2, restart word}, where an env that
// does not restart may leave another word with bit 31 clear in the restart word's place (the slide marks of CodeCells).
enum { RES_STEPPED = 1u, RES_DONE = 2u, RES_STORE_ST = 4u, RES_RESET = 8u };
__device__ __forceinline__ void move_records(int S, const EnvRegs &R, uint32_t flags, uint32_t res, bool done, int winner,
                                             float rw0, float rw1, uint32_t marks, uint4 &rec_st, uint4 &rec_out)
{
    if (done) res |= RES_DONE;
    uint32_t w = marks;
    if (done && (flags & TRON_STEP_AUTORESET)) {                    // ACKTR.py:307-310
        rec_st = restarted_st4(R.nstart, rec_st.w);
        res |= RES_STORE_ST | RES_RESET;
        w = restart_word(S, R.nstart);
    }
    rec_out = make_uint4(res | ((uint32_t)winner << 4), __float_as_uint(rw0), __float_as_uint(rw1), w);
}

// The two cell encodings a move works in, and what a written cell reports (wrote: cell, player, "is a slide tile";
// the words of a move's six cells are ORed into rec_out's last word).
struct BoardCells {                             // the board-owning layout: Tile values (map.py:9-17)
    enum { EMPTY = TRON_EMPTY, WALL = TRON_WALL, P1_BODY = TRON_P1_BODY, P2_BODY = TRON_P2_BODY, P1_HEAD = TRON_P1_HEAD,
           P2_HEAD = TRON_P2_HEAD, P1_SLIDE = TRON_P1_SLIDE, P2_SLIDE = TRON_P2_SLIDE };
    uint32_t *dirty;                            // LDS bitmask of the tile's chunks that the stream writes back to the grid
    uint32_t chunk0;                            // this env's first chunk
    __device__ __forceinline__ uint32_t wrote(int cell, int, bool) const
    {
        const uint32_t ci = chunk0 + (uint32_t)(cell >> 4);
        atomicOr(&dirty[ci >> 5], 1u << (ci & 31u));
        return 0u;
    }
};
struct CodeCells {                              // observation-is-state: player-1 codes (map.py:67-81), see k_obs below
    // a slide tile shows as its player's body: the board image tells them apart by the slide log (see slide_log below)
    enum { EMPTY = 1, WALL = -1, P1_BODY = -2, P2_BODY = -3, P1_HEAD = 10, P2_HEAD = -10, P1_SLIDE = P1_BODY, P2_SLIDE = P2_BODY };
    // slide marks: (cell + 1) of player 1's slide tile | (cell + 1) << 14 of player 2's, 0 = none
    __device__ __forceinline__ uint32_t wrote(int cell, int p, bool slide_tile) const
    {
        return slide_tile ? (uint32_t)(cell + 1) << (14 * p) : 0u;
    }
};

// ------------------------------------------------------------------ the move --
// One lane = one env, against its LDS copy g, in the cell encoding L; every mode (mode None never takes the slide).
// LDS-only, one read round trip.  Leaves its records (move_records).  (Pre-fetching the target cells from HBM before the
// barrier was measured too: +20 VGPRs held across the tile load cost a workgroup per CU and lost.)
template <class L>
__device__ inline void lane_move(const Params &P, const L &layout, unsigned char *g, const EnvRegs &R, const int a[2],
                                 const float u[2], uint32_t flags, uint4 &rec_st, uint4 &rec_out)
{
    const int S = P.S, W = P.W;
    const bool sliding = (P.mode != TRON_MODE_NONE);
    const uint32_t m = R.meta;
    int r[2], c[2];
    unpack_pos(R.pos, r, c);
    bool done = (m & META_DONE) != 0;
    int winner = (int)((m >> 4) & 3u);
    float rw0 = 0.0f, rw1 = 0.0f;
    uint32_t res = 0u, marks = 0u;
    rec_st = make_uint4(R.pos, R.meta, R.eplen, R.tick);

    float thr[2] = {0.0f, 0.0f};
    bool thr_ok[2] = {false, false};
    if (P.mode == TRON_MODE_TEMPER) {
#pragma unroll
        for (int p = 0; p < 2; ++p) temper_threshold(R.envp, p, thr[p], thr_ok[p]);
    }
    if (!done) {
        res |= RES_STEPPED;
        // The <=4 cells the move can look at — first target n[p] and slide landing s[p] of each
        // player (player.py:124-132, game.py:163-178) — are read from the LDS copy in ONE round
        // trip; the write-then-read dependencies between the players are resolved in registers.
        int dr[2], dc[2], n[2], sl[2], tn[2], ts[2];
        bool inb[2], slid[2] = {false, false};
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            action_delta(a[p], dr[p], dc[p]);
            const int nr = r[p] + dr[p], nc = c[p] + dc[p];
            inb[p] = on_board(W, nr, nc);
            n[p] = cell_index(S, nr, nc);
            sl[p] = inb[p] ? cell_index(S, nr + dr[p], nc + dc[p]) : n[p];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            tn[p] = (int)(int8_t)g[n[p]];
            ts[p] = sliding ? (int)(int8_t)g[sl[p]] : (int)L::WALL;
        }
        // cells written so far, in program order; a read sees the latest write to that cell
        int cells[6], vals[6];
        cells[0] = cell_index(S, r[0], c[0]); vals[0] = L::P1_BODY;       // game.py:155-156: heads -> bodies first
        cells[1] = cell_index(S, r[1], c[1]); vals[1] = L::P2_BODY;
#pragma unroll
        for (int k = 2; k < 6; ++k) { cells[k] = cells[k & 1]; vals[k] = vals[k & 1]; }
        auto cell_at = [&](int idx, int before, int upto) {
            int v = before;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (k < upto && cells[k] == idx) v = vals[k];
            return v;
        };

        // game.py:158-178 — advance, optional slide, player order
        int f[2], tf[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            f[p] = n[p];
            tf[p] = tn[p];
            int nr = r[p] + dr[p], nc = c[p] + dc[p];
            // the uniform is consulted only for an in-bounds EMPTY target (game.py:164-165)
            if (sliding && inb[p] && cell_at(n[p], tn[p], 2 + p) == L::EMPTY && slides(P, R, p, u[p], thr[p], thr_ok[p])) {
                cells[2 + p] = n[p];
                vals[2 + p] = (p == 0) ? L::P1_SLIDE : L::P2_SLIDE;
                slid[p] = true;
                f[p] = sl[p];
                tf[p] = ts[p];
                nr += dr[p];
                nc += dc[p];
            }
            r[p] = nr;
            c[p] = nc;
        }

        // game.py:205-214 — collisions in player order; the head is written in every branch
        // (an out-of-bounds head lands on the border WALL cell)
        uint32_t alive = m & 3u;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            alive = collide(alive, p, W, r[p], c[p], cell_at(f[p], tf[p], 4 + p) == L::EMPTY);
            cells[4 + p] = f[p];
            vals[4 + p] = (p == 0) ? L::P1_HEAD : L::P2_HEAD;
        }
        // the writes, in program order (same-lane LDS writes keep their order); fire and forget
#pragma unroll
        for (int k = 0; k < 6; ++k) g[cells[k]] = (unsigned char)vals[k];

        done = settle(alive, r, c, winner);
        step_rewards(P, done, winner, R.eplen, rw0, rw1);

        if (!(done && (flags & TRON_STEP_AUTORESET))) {               // (a restarting env's board is rebuilt whole)
#pragma unroll
            for (int k = 0; k < 6; ++k) marks |= layout.wrote(cells[k], k & 1, (k >> 1) == 1 && slid[k & 1]);
        }
        // a layout whose slide tiles have no value of their own keeps their number in st4.meta (the slide log)
        const uint32_t cnt = ((int)L::P1_SLIDE != (int)L::P1_BODY) ? 0u
                           : ((m >> SLIDE_CNT_SHIFT) & SLIDE_CNT_MASK) + ((marks & 0x3FFFu) ? 1u : 0u) + ((marks >> 14) ? 1u : 0u);
        rec_st = stepped_st4(r, c, pack_meta(alive, done, winner, a[0], a[1], cnt), R.eplen, R.tick);
        res |= RES_STORE_ST;
    }
    move_records(S, R, flags, res, done, winner, rw0, rw1, marks, rec_st, rec_out);
}

// ---------------------------------------------------------------- the kernel --
// One tile of E envs through one step (or one encode); shared by k_tile (one tile per workgroup per
// launch) and k_tile_roll (the persistent rollout, see k_obs_roll).
template <int FMT, bool DO_STEP, bool ALIGNED>
__device__ __forceinline__ void tile_step(const Params &P, int E, uint32_t cpe, uint32_t cpe_magic,
                                          const int8_t *__restrict__ actions, const float *__restrict__ uniforms,
                                          uint32_t flags, void *__restrict__ obs, const StepOut &out, int tile_idx,
                                          unsigned char *smem)
{
    const int G = P.G;
    uint4 *tile = reinterpret_cast<uint4 *>(smem);                  // [E*cpe]
    uint4 *tmpl = tile + (size_t)E * cpe;                           // [cpe] fresh board as chunks
    uint4 *rec_st = tmpl + cpe;                                     // [E] new st4
    uint4 *rec_out = rec_st + E;                                    // [E] flags / rewards / restart word
    uint4 *rec_rs = rec_out + E;                                    // [E] new rs4 (restarted envs)
    float *plane4 = reinterpret_cast<float *>(rec_rs + E);          // [E]
    uint32_t *dirty = reinterpret_cast<uint32_t *>(plane4 + E);     // [ceil(E*cpe/32)] chunk bitmask

    const int tid = threadIdx.x;
    const int e0 = tile_idx * E;
    const int ne = min(E, P.N - e0);
    const int env = e0 + tid;
    const bool mine = tid < ne;
    const uint32_t nchunks = (uint32_t)ne * cpe;
    const int8_t *gtile = P.grid + (size_t)e0 * G;
    const bool sliding = (P.mode != TRON_MODE_NONE);
    const bool autoreset = (flags & TRON_STEP_AUTORESET) != 0u, nonrev = (flags & TRON_STEP_NONREVERSING) != 0u;
    const bool w0 = DO_STEP && tid < WAVE;
    constexpr bool PLANES_BY_ROW = ALIGNED && (FMT == TRON_OBS_PLANES3_F32 || FMT == TRON_OBS_PLANES4_F32);

    STAMP(0);
    // ---- 1: state words first (their latency hides under the tile load), then the tile
    EnvRegs R{};
    if (w0 && mine) {
        const uint4 st = P.st4[env];
        R.pos = st.x; R.meta = st.y; R.eplen = st.z; R.tick = st.w;
        if (autoreset || sliding) {
            const uint4 rs = P.rs4[env];
            R.envp = rs.x; R.episode = rs.y; R.nstart = rs.z; R.nenvp = rs.w;
        }
        if (actions) R.act = reinterpret_cast<const uint16_t *>(actions)[env];
        if (sliding) {
            if (uniforms) {
                const float2 uu = reinterpret_cast<const float2 *>(uniforms)[env];
                R.u0 = uu.x;
                R.u1 = uu.y;
            }
            R.slide = P.slide[env];
        }
    }
    if (FMT == TRON_OBS_PLANES4_F32 && mine) plane4[tid] = (float)degree_slide(P.slide[env]);   // game.py:124-132
    if (DO_STEP && autoreset)
        for (uint32_t d = (uint32_t)tid; d < cpe * 16u; d += BLOCK)
            reinterpret_cast<int8_t *>(tmpl)[d] = (d < (uint32_t)G) ? P.fresh[d] : (int8_t)0;

    int a[2] = {0, 0};
    float u[2] = {R.u0, R.u1};
    for (uint32_t base = 0; base < nchunks; base += DK * BLOCK) {
        uint4 v[DK];
#pragma unroll
        for (int k = 0; k < DK; ++k) {
            const uint32_t i = base + (uint32_t)tid + (uint32_t)k * BLOCK;
            const uint32_t le = chunk_env(i, cpe, cpe_magic);
            const uint32_t c = (i - le * cpe) * 16u;
            if (i < nchunks) v[k] = load_chunk<ALIGNED>(gtile + (size_t)le * G + c);
        }
        if (base == 0u && w0) {
            // the random-number work, in the shadow of the tile load (it needs the counters only)
            for (uint32_t d = (uint32_t)tid; d < (nchunks + 31u) / 32u; d += WAVE) dirty[d] = 0u;
            if (mine) {
                const bool have_actions = actions != nullptr, have_uniforms = uniforms != nullptr;
                if (!have_actions || (sliding && !have_uniforms)) {
                    uint32_t x[4];
                    philox4x32_10((uint32_t)env, R.tick, RNG_STEP, 0u, P.seed, P.stream, x);
                    a[0] = draw_action(x[0], (R.meta >> 8) & 0xFu, nonrev);
                    a[1] = draw_action(x[1], (R.meta >> 12) & 0xFu, nonrev);
                    if (!have_uniforms) {
                        u[0] = (float)(x[2] >> 8) * (1.0f / 16777216.0f);
                        u[1] = (float)(x[3] >> 8) * (1.0f / 16777216.0f);
                    }
                }
                if (have_actions) {
                    a[0] = (int)(R.act & 3u);
                    a[1] = (int)((R.act >> 8) & 3u);
                }
                if (autoreset) {       // speculative: stored only if this env restarts in this launch
                    const NewGame ng = make_game_general(P.seed, P.stream, P.W, P.fair, (uint32_t)env, R.episode + 1u);    // (the straight-line make_game costs these kernels 5-6 VGPRs)
                    rec_rs[tid] = make_uint4(R.nenvp, R.episode + 1u, pack_pos(ng.r1, ng.c1, ng.r2, ng.c2),
                                             pack_envp(ng.w0, ng.w1, ng.degree));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < DK; ++k) {
            const uint32_t i = base + (uint32_t)tid + (uint32_t)k * BLOCK;
            if (i < nchunks) tile[i] = v[k];
        }
    }
    STAMP(1);
    __syncthreads();
    STAMP(2);

    if (DO_STEP) {
        // ---- 2: the move, wave 0, one env per lane, LDS only
        if (w0) {
            uint4 rs = make_uint4(0u, 0u, 0u, 0u), ro = make_uint4(0u, 0u, 0u, 0u);
            if (mine)
                lane_move(P, BoardCells{dirty, (uint32_t)tid * cpe}, reinterpret_cast<unsigned char *>(tile + (size_t)tid * cpe), R, a, u,
                          flags, rs, ro);
            if (tid < E) {
                rec_st[tid] = rs;
                rec_out[tid] = ro;
            }
        }
        STAMP(3);
        __syncthreads();
        STAMP(4);

        // ---- 3a: waves 1-3 write the records out, one kind of array each (lane = env)
        const int wave = tid >> 6, lane = tid & 63;
        if (wave >= 1 && lane < ne) {
            const uint4 ro = rec_out[lane];
            const int genv = e0 + lane;
            if (wave == 1) {
                if (ro.x & RES_STORE_ST) P.st4[genv] = rec_st[lane];
                if (ro.x & RES_RESET) P.rs4[genv] = rec_rs[lane];
            } else if (wave == 2) {
                if (out.done) out.done[genv] = (int8_t)((ro.x & RES_DONE) != 0u);
                if (out.winner) out.winner[genv] = (int8_t)((ro.x >> 4) & 3u);
            } else {
                if (out.reward)
                    reinterpret_cast<float2 *>(out.reward)[genv] = make_float2(__uint_as_float(ro.y), __uint_as_float(ro.z));
            }
        }
#ifndef TRON_STAMPS
        if (out.totals && wave == 3) {
            // {env_steps, p1_wins, p2_wins, draws}: one atomic per counter per workgroup
            const uint32_t f = lane < ne ? rec_out[lane].x : 0u;
            const int wn = ((f & RES_STEPPED) && (f & RES_DONE)) ? (int)((f >> 4) & 3u) : -1;
            const unsigned long long bs = __ballot((f & RES_STEPPED) != 0u);
            const unsigned long long b1 = __ballot(wn == 1), b2 = __ballot(wn == 2), b0 = __ballot(wn == 0);
            if (lane == 0) {
                if (bs) atomicAdd(&out.totals[0], (unsigned long long)__popcll(bs));
                if (b1) atomicAdd(&out.totals[1], (unsigned long long)__popcll(b1));
                if (b2) atomicAdd(&out.totals[2], (unsigned long long)__popcll(b2));
                if (b0) atomicAdd(&out.totals[3], (unsigned long long)__popcll(b0));
            }
        }
#endif
    }

    // ---- 3b: the stream
    for (uint32_t i = (uint32_t)tid; i < nchunks; i += BLOCK) {
        const uint32_t le = chunk_env(i, cpe, cpe_magic);
        const uint32_t k = i - le * cpe;
        const uint32_t c = k * 16u;
        const int nb = min(16, G - (int)c);                               // valid cells in this chunk
        uint4 t = tile[i];
        bool wb = false;
        if (DO_STEP) {
            const uint32_t ri = rec_out[le].w;
            if (is_restart(ri)) {                                          // restarted env: fresh board + heads
                t = tmpl[k];
                const uint32_t d1 = restart_head(ri, 0) - c, d2 = restart_head(ri, 1) - c;
                const uint32_t v1 = (uint32_t)TRON_P1_HEAD << ((d1 & 3u) * 8u);   // EMPTY is 0: OR the head in
                const uint32_t v2 = (uint32_t)TRON_P2_HEAD << ((d2 & 3u) * 8u);   // game.py:90-91
                t.x |= (d1 < 4u ? v1 : 0u) | (d2 < 4u ? v2 : 0u);
                t.y |= (d1 - 4u < 4u ? v1 : 0u) | (d2 - 4u < 4u ? v2 : 0u);
                t.z |= (d1 - 8u < 4u ? v1 : 0u) | (d2 - 8u < 4u ? v2 : 0u);
                t.w |= (d1 - 12u < 4u ? v1 : 0u) | (d2 - 12u < 4u ? v2 : 0u);
                wb = true;
            } else {
                wb = ((dirty[i >> 5] >> (i & 31u)) & 1u) != 0u;
            }
        }
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
        if (wb) store_chunk<ALIGNED>(P.grid + (size_t)(e0 + le) * G + c, nb, w);
        if (PLANES_BY_ROW) {
            if (DO_STEP && wb) tile[i] = t;                                // the plane pass reads the tile from LDS
        } else {
            store_chunk_obs<FMT, ALIGNED>(obs, (size_t)(e0 + le), G, c, nb, w,
                                          (FMT == TRON_OBS_PLANES4_F32) ? plane4[le] : 0.0f);
        }
    }
    if (PLANES_BY_ROW) {
        // f32 planes, 16-byte aligned rows: one wave per env, one lane per 4 cells, so every store
        // instruction writes 64 x 16 contiguous bytes of one plane (per-chunk stores would leave each
        // lane its own 64-byte run: a quarter of every line per instruction)
        constexpr int CH = (FMT == TRON_OBS_PLANES4_F32) ? 4 : 3;
        __syncthreads();
        const int wave = tid >> 6, lane = tid & 63, quads = G >> 2;
        for (int le = wave; le < ne; le += BLOCK / WAVE) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(tile + (size_t)le * cpe);
            float4 *ob = reinterpret_cast<float4 *>(reinterpret_cast<float *>(obs) + (size_t)(e0 + le) * 2u * CH * G);
            const float p4 = (FMT == TRON_OBS_PLANES4_F32) ? plane4[le] : 0.0f;
            for (int j = lane; j < quads; j += WAVE) {
                const uint32_t wd = src[j];
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int ch = 0; ch < CH; ++ch) {
                        const uint32_t bits = (ch < 3) ? plane_bits(ch, p != 0) : 0u;
                        ob[(size_t)(p * CH + ch) * quads + j] =
                            (ch == 3) ? make_float4(p4, p4, p4, p4)
                                      : make_float4(plane_val(bits, wd), plane_val(bits, wd >> 8),
                                                    plane_val(bits, wd >> 16), plane_val(bits, wd >> 24));
                    }
            }
        }
    }
    STAMP(7);
}

template <int FMT, bool DO_STEP, bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void k_tile(Params P, int E, uint32_t cpe, uint32_t cpe_magic,
                                                const int8_t *__restrict__ actions,
                                                const float *__restrict__ uniforms, uint32_t flags,
                                                void *__restrict__ obs, StepOut out, int tile0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    tile_step<FMT, DO_STEP, ALIGNED>(P, E, cpe, cpe_magic, actions, uniforms, flags, obs, out, (int)blockIdx.x + tile0, smem);
}

typedef __attribute__((address_space(4))) const unsigned char kernarg_t;    // the kernel-argument segment (constant address space: scalar loads)
__device__ __forceinline__ void load_params(Params &p, kernarg_t *q)       // Params is every rollout kernel's first argument
{
    // one block copy straight from the constant address space (wide scalar loads).  Measured alternatives, same box: word by
    // word, or through a generic pointer, the rollout is 8 % SLOWER than with the parameters simply kept live.
    __builtin_memcpy(&p, q, sizeof(Params));
}

// Persistent rollout on the board-owning layout: the COMPATIBILITY PATH of tron_rollout_random — every mode, format and
// side the observation-is-state kernels (k_obs_roll, k_obs_roll_walk, k_obs_roll_slide) do not take; correct, not tuned.
// tile_step in k_obs_roll's loop of steps and tiles.
template <int FMT, bool ALIGNED>
__global__ __launch_bounds__(BLOCK) void k_tile_roll(Params P, int E, uint32_t cpe, uint32_t cpe_magic, uint32_t flags,
                                                     void *__restrict__ obs, StepOut out, int k_steps, int ntiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long acc[4];           // see k_obs_roll
    StepOut lo = out;
    if (out.totals) {
        if (threadIdx.x < 4) acc[threadIdx.x] = 0ull;
        lo.totals = acc;
        __syncthreads();
    }
    // (Params stays live across the loop here: re-read per step as in k_obs_roll, this kernel goes from 97-106 to 135-141 VGPRs —
    // three waves per SIMD instead of four — and temper mode from 2.58 to 2.23 G env-steps/s)
    for (int s = 0; s < k_steps; ++s)
        for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
            tile_step<FMT, true, ALIGNED>(P, E, cpe, cpe_magic, nullptr, nullptr, flags, obs, lo, t, smem);
            __syncthreads();
        }
    if (out.totals && threadIdx.x < 4 && acc[threadIdx.x]) atomicAdd(&out.totals[threadIdx.x], acc[threadIdx.x]);
}

// ------------------------------------------------- observation-is-state kernel --
// Mode None, int8 code observations, even board side.  There are no slide tiles in this mode,
// so the player-1 code plane (map.py:67-81) is a lossless image of the board.  The caller
// attaches its [N][2][G] observation buffer once (tron_attach_obs_state) and that buffer IS the
// env state: a step reads the player-1 plane (G bytes per env) and rewrites both planes (2G) —
// exactly the algorithmic traffic, no dirty-chunk write-back, no rewrite of restarted boards.
// Same three phases as k_tile; differences: the tile holds player-1 codes, the move works in
// code space (EMPTY is 1; bodies -2 / -3; heads 10 / -10), the player-2 plane is the
// swap_codes4 LUT of the player-1 plane, and wave 1 draws the speculative next start so it runs
// beside wave 0's action Philox instead of after it.
// The move of mode None in code space (CodeCells): no slide, so two target cells in one LDS round trip and four writes —
// the shape k_obs is tuned around; the sliding modes on this layout go through lane_move<CodeCells>.
__device__ inline void lane_move_codes(const Params &P, unsigned char *g, const EnvRegs &R, const int a[2],
                                       uint32_t flags, uint4 &rec_st, uint4 &rec_out)
{
    typedef CodeCells C;
    const int S = P.S, W = P.W;
    int r[2], c[2];
    unpack_pos(R.pos, r, c);
    bool done = (R.meta & META_DONE) != 0;
    int winner = (int)((R.meta >> 4) & 3u);
    float rw0 = 0.0f, rw1 = 0.0f;
    uint32_t res = 0u;
    rec_st = make_uint4(R.pos, R.meta, R.eplen, R.tick);

    if (!done) {
        res |= RES_STEPPED;
        int old[2], f[2], tf[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            int dr, dc;
            action_delta(a[p], dr, dc);
            old[p] = cell_index(S, r[p], c[p]);
            r[p] += dr;
            c[p] += dc;
            f[p] = cell_index(S, r[p], c[p]);
        }
        tf[0] = (int)(int8_t)g[f[0]];                                  // one LDS round trip for both targets
        tf[1] = (int)(int8_t)g[f[1]];
        plain_targets(old, f, tf, (int)C::P1_BODY, (int)C::P2_BODY, (int)C::P1_HEAD);
        uint32_t alive = R.meta & 3u;
#pragma unroll
        for (int p = 0; p < 2; ++p) alive = collide(alive, p, W, r[p], c[p], tf[p] == C::EMPTY);
        // writes in the reference's order: bodies, then P1's head, then P2's (an out-of-bounds
        // head lands on the border WALL cell; a same-cell head-on leaves P2's head)
        g[old[0]] = (unsigned char)C::P1_BODY;
        g[old[1]] = (unsigned char)C::P2_BODY;
        g[f[0]] = (unsigned char)C::P1_HEAD;
        g[f[1]] = (unsigned char)C::P2_HEAD;

        done = settle(alive, r, c, winner);
        step_rewards(P, done, winner, R.eplen, rw0, rw1);
        rec_st = stepped_st4(r, c, pack_meta(alive, done, winner, a[0], a[1]), R.eplen, R.tick);
        res |= RES_STORE_ST;
    }
    move_records(S, R, flags, res, done, winner, rw0, rw1, 0u, rec_st, rec_out);
}

// ---- the sliding modes ("ice", "temper") on the observation-is-state layout ---------------------------------------------
// A slide leaves a P1_slide / P2_slide tile behind (game.py:163-178) that Map.color shows as that player's body
// (map.py:67-81): the dynamics never tell the two apart (a cell is EMPTY or it is not), only the board image does
// (tron_get_grid).  So the player-1 code plane carries the game here too, and the slide marks go to a per-env LOG —
// entry = cell | player << 15, appended by the step that makes the mark (2 bytes, only when somebody slides), their
// number in st4.meta bits 16-29 (a restart rewrites meta: the log empties by itself) — which tron_get_grid replays:
// a logged cell that still holds its player's body code is a slide tile.  The board-owning layout wrote every
// dirty 16-byte chunk of the board back as a partial line instead: 153 MB per step against 121 (profiles/r04_temper_pmc.txt).
__device__ __forceinline__ uint16_t *slide_log(const Params &P)
{
    return reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(P.slide) + (((size_t)P.N * 8u + 255u) & ~(size_t)255u));
}
__host__ __device__ __forceinline__ int slide_log_len(int W) { return W * W; }   // a mark takes a cell of its own

// One tile of E envs through one step; `smem` is the workgroup's dynamic LDS.  Shared by k_obs (one
// tile per workgroup per launch) and k_obs_roll_walk / k_obs_roll_slide (workgroups that keep stepping their own tiles).
// keep_tile (k_obs_roll_slide, TRON_ROLLOUT_RESIDENT): the tile's LDS copy is left exactly as the next step needs
// it (restarted boards are written back to it); have_tile: it already is, so the tile is not loaded again.
template <bool DO_STEP, bool SLIDING = false>
__device__ __forceinline__ void obs_tile(const Params &P, int E, uint32_t cpe, uint32_t cpe_magic,
                                         const int8_t *__restrict__ actions, uint32_t flags, const StepOut &out,
                                         int tile_idx, unsigned char *smem, bool have_tile = false, bool keep_tile = false,
                                         const float *__restrict__ uniforms = nullptr)
{
    const int G = P.G;
    uint4 *tile = reinterpret_cast<uint4 *>(smem);                  // [E*cpe] player-1 codes
    uint4 *tmpl = tile + (size_t)E * cpe;                           // [cpe] fresh board as player-1 codes
    uint4 *rec_st = tmpl + cpe;                                     // [E]
    uint4 *rec_out = rec_st + E;                                    // [E]
    uint4 *rec_rs = rec_out + E;                                    // [E] new rs4 (restarted envs)
    uint4 *rs_in = rec_rs + E;                                      // [E] rs4 as loaded by wave 1

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int e0 = tile_idx * E;
    const int ne = min(E, P.N - e0);
    const uint32_t nchunks = (uint32_t)ne * cpe;
    int8_t *otile = P.obs_state + (size_t)e0 * 2u * G;              // this tile's [ne][2][G] planes
    const bool autoreset = (flags & TRON_STEP_AUTORESET) != 0u, nonrev = (flags & TRON_STEP_NONREVERSING) != 0u;
    const bool mine = lane < ne;
    const int env = e0 + lane;

    STAMP(0);
    // ---- 1: state words (wave 0: st4, wave 1: rs4), then the tile
    EnvRegs R{};
    uint4 rs = make_uint4(0u, 0u, 0u, 0u);
    if (DO_STEP && mine) {
        if (wave == 0) {
            const uint4 st = P.st4[env];
            R.pos = st.x; R.meta = st.y; R.eplen = st.z; R.tick = st.w;
            if (actions) R.act = reinterpret_cast<const uint16_t *>(actions)[env];
            if (SLIDING) {                                            // the slide's rate: this env's scalars (game.py:83-88,100-112)
                R.envp = P.rs4[env].x;
                R.slide = P.slide[env];
                if (uniforms) {
                    const float2 uu = reinterpret_cast<const float2 *>(uniforms)[env];
                    R.u0 = uu.x;
                    R.u1 = uu.y;
                }
            }
        } else if (wave == 1 && autoreset) {
            rs = P.rs4[env];
        }
    }
    if (DO_STEP && autoreset)
        for (uint32_t d = (uint32_t)tid; d < cpe * 16u; d += BLOCK)
            reinterpret_cast<int8_t *>(tmpl)[d] = (d < (uint32_t)G) ? (P.fresh[d] == TRON_EMPTY ? (int8_t)1 : (int8_t)-1) : (int8_t)0;

    int a[2] = {0, 0};
    float u[2] = {R.u0, R.u1};
    for (uint32_t base = 0; base < nchunks; base += DK * BLOCK) {
        uint4 v[DK];
#pragma unroll
        for (int k = 0; k < DK; ++k) {
            const uint32_t i = base + (uint32_t)tid + (uint32_t)k * BLOCK;
            const uint32_t le = chunk_env(i, cpe, cpe_magic);
            const uint32_t c = (i - le * cpe) * 16u;
            if (i < nchunks && !have_tile) v[k] = load_chunk<true>(otile + (size_t)le * 2u * G + c);   // player-1 plane
        }
        if (base == 0u && DO_STEP && mine) {
            // random-number work in the shadow of the tile load: wave 0 the actions (and slide uniforms), wave 1 the next start
            if (wave == 0) {
                if (!actions || (SLIDING && !uniforms)) {
                    uint32_t x[4];
                    philox4x32_10((uint32_t)env, R.tick, RNG_STEP, 0u, P.seed, P.stream, x);
                    a[0] = draw_action(x[0], (R.meta >> 8) & 0xFu, nonrev);
                    a[1] = draw_action(x[1], (R.meta >> 12) & 0xFu, nonrev);
                    if (SLIDING && !uniforms) {
                        u[0] = (float)(x[2] >> 8) * (1.0f / 16777216.0f);
                        u[1] = (float)(x[3] >> 8) * (1.0f / 16777216.0f);
                    }
                }
                if (actions) {
                    a[0] = (int)(R.act & 3u);
                    a[1] = (int)((R.act >> 8) & 3u);
                }
            } else if (wave == 1 && autoreset) {
                rs_in[lane] = rs;
                const NewGame ng = make_game_general(P.seed, P.stream, P.W, P.fair, (uint32_t)env, rs.y + 1u);
                rec_rs[lane] = make_uint4(rs.w, rs.y + 1u, pack_pos(ng.r1, ng.c1, ng.r2, ng.c2),
                                          pack_envp(ng.w0, ng.w1, ng.degree));
            }
        }
#pragma unroll
        for (int k = 0; k < DK; ++k) {
            const uint32_t i = base + (uint32_t)tid + (uint32_t)k * BLOCK;
            if (i < nchunks && !have_tile) tile[i] = v[k];
        }
    }
    STAMP(1);
    __syncthreads();
    STAMP(2);

    if (DO_STEP) {
        // ---- 2: the move, wave 0, one env per lane, LDS only
        if (wave == 0) {
            uint4 rst = make_uint4(0u, 0u, 0u, 0u), ro = make_uint4(0u, 0u, 0u, 0u);
            if (mine) {
                if (autoreset) R.nstart = rs_in[lane].z;
                unsigned char *g = reinterpret_cast<unsigned char *>(tile + (size_t)lane * cpe);
                if (SLIDING) lane_move(P, CodeCells{}, g, R, a, u, flags, rst, ro);
                else lane_move_codes(P, g, R, a, flags, rst, ro);
            }
            if (lane < E) {
                rec_st[lane] = rst;
                rec_out[lane] = ro;
            }
        }
        STAMP(3);
        __syncthreads();
        STAMP(4);

        // ---- 3a: waves 1-3 write the records out (lane = env)
        if (wave >= 1 && mine) {
            const uint4 ro = rec_out[lane];
            if (wave == 1) {
                if (ro.x & RES_STORE_ST) P.st4[env] = rec_st[lane];
                if (ro.x & RES_RESET) P.rs4[env] = rec_rs[lane];
            } else if (wave == 2) {
                if (out.done) out.done[env] = (int8_t)((ro.x & RES_DONE) != 0u);
                if (out.winner) out.winner[env] = (int8_t)((ro.x >> 4) & 3u);
            } else {
                if (out.reward)
                    reinterpret_cast<float2 *>(out.reward)[env] = make_float2(__uint_as_float(ro.y), __uint_as_float(ro.z));
                if (SLIDING && ro.w && !is_restart(ro.w)) {           // this step's slide marks (CodeCells) go to the env's log
                    const uint32_t m0 = ro.w & 0x3FFFu, m1 = ro.w >> 14;
                    uint32_t at = ((rec_st[lane].y >> SLIDE_CNT_SHIFT) & SLIDE_CNT_MASK) - (m0 ? 1u : 0u) - (m1 ? 1u : 0u);
                    uint16_t *lg = slide_log(P) + (size_t)env * slide_log_len(P.W);
                    if (m0) lg[at++] = (uint16_t)(m0 - 1u);
                    if (m1) lg[at] = (uint16_t)((m1 - 1u) | 0x8000u);
                }
            }
        }
#ifndef TRON_STAMPS
        if (out.totals && wave == 3) {
            const uint32_t f = mine ? rec_out[lane].x : 0u;
            const int wn = ((f & RES_STEPPED) && (f & RES_DONE)) ? (int)((f >> 4) & 3u) : -1;
            const unsigned long long bs = __ballot((f & RES_STEPPED) != 0u);
            const unsigned long long b1 = __ballot(wn == 1), b2 = __ballot(wn == 2), b0 = __ballot(wn == 0);
            if (lane == 0) {
                if (bs) atomicAdd(&out.totals[0], (unsigned long long)__popcll(bs));
                if (b1) atomicAdd(&out.totals[1], (unsigned long long)__popcll(b1));
                if (b2) atomicAdd(&out.totals[2], (unsigned long long)__popcll(b2));
                if (b0) atomicAdd(&out.totals[3], (unsigned long long)__popcll(b0));
            }
        }
#endif
    } else {
        return;                                                        // nothing to re-encode: the planes are the state
    }

    // ---- 3b: the stream: both planes of every chunk
    for (uint32_t i = (uint32_t)tid; i < nchunks; i += BLOCK) {
        const uint32_t le = chunk_env(i, cpe, cpe_magic);
        const uint32_t k = i - le * cpe;
        const uint32_t c = k * 16u;
        const int nb = min(16, G - (int)c);
        uint4 t = tile[i];
        const uint32_t ri = rec_out[le].w;
        if (is_restart(ri)) {                                          // restarted env: fresh board + heads
            t = tmpl[k];
            const uint32_t d1 = restart_head(ri, 0) - c, d2 = restart_head(ri, 1) - c;
            // the head cells are EMPTY (code 1) in the template: XOR turns 1 into 10 / -10 (game.py:90-91)
            const uint32_t v1 = (uint32_t)(0x01 ^ 0x0A) << ((d1 & 3u) * 8u), v2 = (uint32_t)(0x01 ^ 0xF6) << ((d2 & 3u) * 8u);
            t.x ^= (d1 < 4u ? v1 : 0u) ^ (d2 < 4u ? v2 : 0u);
            t.y ^= (d1 - 4u < 4u ? v1 : 0u) ^ (d2 - 4u < 4u ? v2 : 0u);
            t.z ^= (d1 - 8u < 4u ? v1 : 0u) ^ (d2 - 8u < 4u ? v2 : 0u);
            t.w ^= (d1 - 12u < 4u ? v1 : 0u) ^ (d2 - 12u < 4u ? v2 : 0u);
            if (keep_tile) tile[i] = t;
        }
        const uint32_t w1[4] = {t.x, t.y, t.z, t.w};
        const uint32_t w2[4] = {swap_codes4(t.x), swap_codes4(t.y), swap_codes4(t.z), swap_codes4(t.w)};
        int8_t *o1 = otile + (size_t)le * 2u * G + c;
        store_chunk<true>(o1, nb, w1);
        store_chunk<true>(o1 + G, nb, w2);
    }
    STAMP(7);
}

template <bool DO_STEP>
__global__ __launch_bounds__(BLOCK) void k_obs(Params P, int E, uint32_t cpe, uint32_t cpe_magic,
                                               const int8_t *__restrict__ actions, uint32_t flags, StepOut out,
                                               int tile0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    obs_tile<DO_STEP>(P, E, cpe, cpe_magic, actions, flags, out, (int)blockIdx.x + tile0, smem);
}
// ... and in the sliding modes (own kernels: mode None's stay as they were, instruction for instruction)
__global__ __launch_bounds__(BLOCK) void k_obs_slide(Params P, int E, uint32_t cpe, uint32_t cpe_magic, const int8_t *__restrict__ actions,
                                                     const float *__restrict__ uniforms, uint32_t flags, StepOut out, int tile0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    obs_tile<true, true>(P, E, cpe, cpe_magic, actions, flags, out, (int)blockIdx.x + tile0, smem, false, false, uniforms);
}

// load_params for a loop that must not issue a vector-memory load: the source is typed as 32-bit words, so the copy is
// known to be dword-aligned and becomes s_load_dwordx4/x8 (lgkmcnt).  Through kernarg_t's byte pointer the same copy is
// taken for unaligned and comes out as global_load_dwordx4 + v_readfirstlane: vmcnt, behind every store the wave has issued.
typedef __attribute__((address_space(4))) const uint32_t kernarg_words_t;
__device__ __forceinline__ void load_params_scalar(Params &p, kernarg_t *kp)
{
    kernarg_words_t *q = reinterpret_cast<kernarg_words_t *>(kp);
    asm volatile("" : "+s"(q));                                     // (a pointer the compiler cannot see through)
    __builtin_memcpy(&p, q, sizeof(Params));
}

// ---- the boards of k_obs_roll in LDS: 4 bits per cell ---------------------------------------------------------------------
// The six player-1 codes of mode None (1, -1, -2, -3, 10, -10) have distinct low nibbles (1, F, E, D, A, 6), so a cell is kept
// as its code's low nibble, cell j of a 16-cell chunk in bits 4 (j & 7) of dword j >> 3: a chunk is two dwords, a 24x24
// board 43 chunks = 344 bytes.  The code comes back as nibble | 0xF0 where the nibble's bit 2 is set (F, E, D, 6: the
// negative ones); a padding nibble 0 (cells past G in the last chunk) comes back as 0.
constexpr uint32_t NIB_EMPTY = 0x1u, NIB_WALL = 0xFu, NIB_P1_BODY = 0xEu, NIB_P2_BODY = 0xDu, NIB_P1_HEAD = 0xAu, NIB_P2_HEAD = 0x6u;
__device__ __forceinline__ uint32_t pack_codes8(uint32_t w0, uint32_t w1)       // 8 code bytes -> 8 nibbles
{
    const uint32_t a = w0 & 0x0F0F0F0Fu, b = w1 & 0x0F0F0F0Fu;
    const uint32_t ta = a | (a >> 4), tb = b | (b >> 4);                        // bytes 0 and 2 hold two nibbles each
    return (ta & 0xFFu) | ((ta >> 8) & 0xFF00u) | ((tb & 0xFFu) << 16) | ((tb << 8) & 0xFF000000u);
}
// No multiply: the code of a nibble is a byte LUT on its low three bits (0 -> 0, 1 -> 1, 2 (A) -> 0x0A, 5 (D) -> 0xF5,
// 6 (6 / E) -> 0xF6, 7 (F) -> 0xF7) with the nibble's bit 3 put back on top.  The same routine serves both players' nibbles.
constexpr uint32_t EXPAND_LO = pack4(0, 1, 0x0A, 0), EXPAND_HI = pack4(0, 0xF5, 0xF6, 0xF7);
__device__ __forceinline__ void expand_codes8(uint32_t p, uint32_t &w0, uint32_t &w1)   // 8 nibbles -> 8 code bytes
{
    const uint32_t q = p >> 4;                                                  // p: even cells, q: odd cells
    const uint32_t lo = __builtin_amdgcn_perm(EXPAND_HI, EXPAND_LO, p & 0x07070707u) | (p & 0x08080808u);
    const uint32_t hi = __builtin_amdgcn_perm(EXPAND_HI, EXPAND_LO, q & 0x07070707u) | (q & 0x08080808u);
    w0 = __builtin_amdgcn_perm(hi, lo, 0x05010400u);
    w1 = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
}
// Player-2 nibbles from player-1 nibbles, eight cells at once (swap_codes4 in nibble space): bodies E <-> D are ^ 3, heads
// A <-> 6 are ^ 0xC, and 1, F and the padding 0 stay.  With the nibble's bits b3..b0, a head is b3 ^ b2 and a body is
// b3 & b2 & (b1 ^ b0).
__device__ __forceinline__ uint32_t swap_nibbles8(uint32_t p)
{
    const uint32_t s = p >> 1;
    const uint32_t x = p ^ s;                                                   // bit 0: b1 ^ b0, bit 2: b3 ^ b2 (bit 3 is not used)
    const uint32_t body = ((p & s) >> 2) & 0x11111111u;                         // bit 0: b3 & b2
    const uint32_t z = x & (body | 0x44444444u);                                // bit 0: a body, bit 2: a head
    return p ^ z ^ (z << 1);
}

// The steps of a persistent launch (k_obs_roll): ONE LANE = ONE ENV for the whole launch, and a wave owns its envs from the
// prologue to the epilogue.  Nobody else touches an env's planes or state words during the launch, and nobody can read them
// before it ends, so everything a step reads or writes is carried from the step before: the env's state, rs4 and the
// block's action bytes in the lane's registers, the board in the lane's own region of LDS (4 bits per cell, above).
// The state is carried DECODED and in CELL SPACE: the two heads' indices into the padded board (no r and no c: the index
// determines both, and collide / settle have cell-space overloads with the argument, tron_device.hpp), the LDS address
// and nibble shift of each head's dword, alive, done, winner, the two last actions + 1 (the non-reversing policy), eplen
// and tick (deriving the two counters in the epilogue instead was built and taken out again: alone it lengthened the
// stamped step, profiles/r31_rollout_ab.txt).  The prologue unpacks st4 once; a step moves a head's cell by +-1 or
// +-S — one signed byte of the launch-uniform word cell_deltas(S), picked by the action — and derives the rest of the new
// head from that, and the old heads' cells and addresses are simply the ones the step before computed; a restart
// sets them all from the next game's start cells, which the start ring holds IN CELL SPACE (start_cells_word: roll_cell
// of each player, 16 + 16 bits; rs4.nstart is converted once by the prologue and back by the epilogue of a lane that
// restarted); the epilogue divides r and c back out of the cells (one division by S per env and
// launch) and packs st4 once, under st_dirty, into the bytes stepped_st4 / restarted_st4 of the env's last event would
// have left.  A block's action bytes are consumed once where they are loaded, so no step waits for them: between a
// step's last LDS operation and the next step's reads stands no s_waitcnt, and the restart's start-ring read is waited
// for where rs.z is next used, the lane's next restart.  The helper reads st and rs as loaded.  The game
// wave does the move, a restarted env's board, the records and the lane's tally of the totals; what is random — the actions
// of every step and the starts of every restarted env's next game — its helper wave draws ahead of it into rings in LDS
// (roll_helper above: the rings, their invariants and the barriers).  The step loop has ONE workgroup barrier per block of
// ROLL_R steps and none inside a block; no lane touches another lane's board, and the game waves of a workgroup share the
// fresh-board template only, built in the prologue.  Memory is read in the prologue only and the planes are written in the epilogue only: the loop holds
// no global load, no s_waitcnt vmcnt and no plane store (with every CU storing 8 scattered 16-byte chunks per env-step the
// shared store path set the launch time: profiles/r10_rollout_ab.txt, r11_rollout_ab.txt).  Of the parameters the loop
// needs S and W alone, two SGPRs for the whole launch; REC re-reads N and the reward table per step with scalar loads
// (load_params_scalar).  A block's steps are an inner loop of their own: the block-start branch is outside it.
// What the caller sees: when the launch completes on its stream the buffer holds the observations of its last step, exactly
// the bytes one store per step would have left; until a wave's epilogue its envs' planes hold what the launch began with.
// LDS: an env's board takes 2 cpe + 1 dwords — odd, so that the same dword of the boards of the 64 lanes falls on 64
// different banks (any power-of-two bank count) — and 65 536 boards of 24x24 are 22.8 MB: the whole batch is resident at
// once, the launch is one round (rollout_persistent).
// Three 64-bit chunk masks per env (cpe <= 64: boards up to 30x30; the host sends wider ones to k_obs_roll_walk).
//   mask:  the chunks of the player-1 plane that may differ from the fresh-board template.
//   stale: the chunks whose bytes in the lane's LDS board are garbage (a finished game's trail) and whose content IS the
//          template.
//   dirty: the chunks whose bytes in memory may differ from the env's board — 0 after the prologue.
// Invariants: stale & mask == 0; a chunk outside mask | stale holds the template in LDS; stale is a subset of dirty.
// The chunks of the two heads of a game in progress are in mask, and from the launch's first step on in dirty: a head
// cell is not the template's EMPTY, so the entry (compare or entry mask) has its chunk in mask; a move puts the NEW
// heads' chunks into both, a restart its heads; and dirty takes the entry heads' chunks once, behind the prologue (a
// chunk stored for that alone is stored with the bytes memory has).  So a move marks its two new chunks and no more.
// The prologue builds mask by comparing what it reads with the template, whoever wrote it (every writer of the API leaves the
// player-2 plane the swap_codes4 image of the player-1 plane, and the caller never writes the buffer); stale starts at 0.
// Nothing is compared in the loop.
// A step has ONE body and one LDS round trip.  A restart is due in the step its game finishes in (the lane has made its move)
// and, for an env that entered the launch finished, in the launch's first step without a move.  The round trip reads, for
// every lane: the template's two dwords of the two START chunks of the env's next game (rs.z is in registers since the
// restart before) and the start ring's word of the game after that one — the next game's kit, dropped by a lane that does
// not restart —, and for a moving lane the two new heads' cells, one dword each (the old heads' cells are only overwritten),
// and the template's chunks of theirs.  Only a new head can lie in a stale chunk (the old heads' chunks are in mask);
// where it does, the cell's nibble is taken from the template.  plain_targets and collide so see what the wiped board would
// have shown, an out-of-bounds head on the border wall and both heads in one stale chunk included.
// Behind the judgement the board work is one piece of code: its two cells are the new heads for a move that goes on and the
// start cells for a restart; a chunk that must be refreshed (a new head's stale chunk; both of a restart's chunks, always)
// gets the template's two dwords and leaves stale, THEN the cell writes go on top: the old heads' body nibbles (a move
// alone) and the two head nibbles, four ds_mskor_b32 (lds_set_nibble: memory = (memory & ~mask) | data on the cell's dword)
// in the reference's order.  A lane's LDS operations execute in order, so cells that share a dword need no merging in
// registers and two heads in one chunk or one dword land on the template bytes whichever chunk write came last.  The two
// chunks are marked in mask and dirty.  A restart wipes nothing: in front of the shared part it sets dirty |= mask,
// stale |= mask, mask = 0, so that the shared part leaves stale = (stale | mask) & ~heads, dirty |= mask | heads,
// mask = heads.  Most of a trail's chunks are never looked at again before the next restart; the few that are, are known at
// the moment a move looks at them.  The restart's tail sets the state words and takes the ring's word: it waits for nothing.
// A lane writes only its own board in the loop, so the loop needs no fence and no wave barrier.
// The epilogue stores dirty & (mask | mask0), mask0 being the mask the prologue built: a chunk outside both is the template
// (in LDS or as a stale chunk) and was the template in memory when the launch began, so the bytes are equal.  That filter
// keeps the set small: a third of the env-steps are restarts at fresh places, so over 64 steps dirty grows to nearly every
// chunk of a 24x24 board, while mask | mask0 is two episodes' trails.  A stored chunk that is still stale — one of mask0 that
// no later game touched — is stored FROM THE TEMPLATE: bit 12 of its list entry selects the source in the trip body (about
// three instructions per entry written and per trip; the alternative, the per-lane copy loop once per launch over
// stale & mask0 in front of the list, is 17 per chunk of the wave's slowest lane).  The stores go through a wave-wide list,
// because the lanes' counts differ: each lane puts its (source, lane, chunk) entries, two bytes each, into the wave's list
// in LDS at the prefix sum of the lanes' counts; then lane l of trip t takes entry 64 t + l, whoever owns it: one LDS read
// from the owner's board or the template, the player-2 nibbles (swap_nibbles8), four multiply-free expansions and two
// 16-byte stores.  The list is in (lane, chunk) order, so neighbouring lanes mostly store neighbouring chunks of one env.
// Lanes read boards they do not own here; LDS operations of one wave execute in order, and a wavefront-scope fence in front
// of the trips keeps the compiler to that order (no barrier, no wait on memory).  The plane's short last chunk has a branch
// of its own before the list, with the same choice of source.
// The next game of a restarted env.  CONTRACT: no step of mode None reads rs4.envp or rs4.nenvp (the weights and the degree
// act in the sliding modes only, and this kernel is launched for mode None alone: tron_rollout_random sends every other
// mode to k_obs_roll_slide / k_tile_roll).  They matter as the bytes of rs4 the epilogue stores, so the loop draws what a
// step does read and no more: a restart moves rs4.episode on and draws rs4.nstart with make_game_starts — one Philox block
// and four draws in a line (two blocks with `fair`), whose lanes go on into the general routine only when their two
// starts clash, drawn by the helper since round 14 and read from its ring at the restart's ordinal — and counts the env's
// restarts (the epilogue asks: 0, 1, or two and more).  The epilogue then sets the two words from the
// final episode e: nenvp is make_game(env, e)'s; envp is untouched without a restart, the nenvp the prologue read after
// one, make_game(env, e - 1)'s after two and more — what rotating the words at every restart left there, tron_set_weight_
// degree's values in envp until the first restart included.  Both through the full make_game, clash path and all.  A third
// of the env-steps of a 24x24 batch are restarts, so some lane of a wave restarts in nearly every step and the wave ran
// make_game's second block, with a third of its lanes active, in nearly every step (profiles/r13_rollout_ab.txt).
// An env that restarts in the step it finishes in skips the move's four cell writes and its refreshes: its trail goes stale
// by the mask as it was before the move.  st4 / rs4 are written by the epilogue as well (same bytes as one store per step
// leaves behind).
// The records.  REC (k_obs_roll_tape_rec, tron_rollout_actions_records) stores what every step computes anyway — done,
// winner and, when out.reward is asked for, the two rewards — into the caller's step-major tapes: out.done / out.winner are
// int8[k_steps][N], out.reward float2[k_steps][N], the launch's own first step at row 0, any of them null.  The row's
// offset is wave-uniform and is carried forward by N per step (no multiply in the loop); a lane adds its env: per wave
// and step 64 contiguous bytes of done, 64 of winner, 512 of reward.  The stores are fire-and-forget: the loop still loads
// nothing from memory and waits for nothing, a null tape costs a uniform branch, a lane without an env stores nothing and the
// helper waves store no records.  Row s is what the s-th tron_step_encode with autoreset records, an env that is finished
// when the step begins included: done 1, its old winner, rewards 0.
// Without REC (k_obs_roll, k_obs_roll_tape) the loop holds no record store, no step_rewards and no load of the reward
// table: tron_rollout_random and tron_rollout_actions pass out.totals only, and a call that asks for records runs the REC
// instantiation.  tron_rollout_random always sets TRON_STEP_AUTORESET, and so do the tape calls: the
// !autoreset branches below are run by no caller and no test.
// ---- the helper wave of k_obs_roll -------------------------------------------------------------------------------------------
// A launch's steps come in blocks of ROLL_R.  Per game wave the helper keeps two rings in LDS:
//   actions  [2][64] x ROLL_R bytes: action_byte of step s of env `lane` is byte s % ROLL_R of slot (s / ROLL_R) & 1
//   starts   [2 ROLL_R][64] dwords: make_game_starts(env, episode0 + j), the start of the game the env's j-th restart of
//            the launch draws, in slot (episode0 + j) % (2 ROLL_R): the slot of an ABSOLUTE episode, so that a ring image
//            still means something to the next launch, whose episode0 has moved on (Hand-off below).  A slot holds the
//            start IN CELL SPACE: start_cells_word, roll_cell of player 1 | roll_cell of player 2 << 16.  Every writer of
//            a slot converts once (the top-up loop here, the game wave's ROLL_GAME_STARTS draws); the restart reads
//            cells and converts nothing, and neither does a handed entry: hand[0 .. 2 ROLL_R) are slots as they are.
//            The format is the blob's own, written and read by this library alone, within one process.
// and reads one word per env and block, counts[64]: the env's restarts so far.
constexpr int ROLL_R = 8;
// A launch flag of the host's own (rollout_wave), beside the TRON_STEP_* bits: every env's entry mask describes its planes.
constexpr uint32_t ROLL_ENTRY_MASKED = 0x80000000u;
// Behind a masked entry the game wave is at P within 5 us and its helper, with 16 Philox blocks to draw, is not (stamps:
// profiles/r18_rollout_ab.txt).  The game wave then draws the last ROLL_GAME_STARTS ordinals of block 0 itself, after its
// gather; with 2 the two roles meet at P (0: the helper is 2.8 us late in every pair, 4: the game wave is 1.4 us late).
constexpr int ROLL_GAME_STARTS = 2;
// The second flag of the host's own: the launch before this one on the handle handed over its helper's rings (roll_helper:
// Hand-off).  hand is [ROLL_HAND_DWORDS][N] dwords in the handle's blob, word-major, so that a wave's 64 envs are 256
// contiguous bytes per word: the 2 ROLL_R slots of the start ring, the two dwords of the next launch's block-0 action
// bytes, and the highest absolute episode the ring holds.  No action byte is 0xFF (action_byte: bits 4-5 and 6-7 are
// __umulhi(x, 3) <= 2), so a second action dword of ROLL_HAND_NO_ACTIONS says "starts only" (a tape launch's hand-off).
constexpr uint32_t ROLL_ENTRY_HANDED = 0x40000000u;
constexpr int ROLL_HAND_DWORDS = 2 * ROLL_R + 3;
constexpr uint32_t ROLL_HAND_NO_ACTIONS = 0xFFFFFFFFu;
constexpr size_t ROLL_RING_DWORDS = 4 * WAVE + 2 * ROLL_R * WAVE + 2 * WAVE;
static_assert(ROLL_R == 8 && TRON_ROLLOUT_CHUNK % ROLL_R == 0, "a block's action bytes are one qword; blocks tile a launch");
#ifdef TRON_STAMPS
static_assert(ROLL_HSTAMPS == 4 + 2 * (TRON_ROLLOUT_CHUNK / ROLL_R), "two helper stamps per block barrier");
#endif

// The wave's share of out.totals: the lanes' byte counts (steps, player-1 wins, player-2 wins, draws; at most 255 each)
// summed over the wave into the uniform counters.
__device__ __forceinline__ void roll_flush_tally(uint32_t &tally, uint32_t &n_steps, uint32_t &n_w1, uint32_t &n_w2, uint32_t &n_draw)
{
    uint32_t a = tally & 0x00FF00FFu, b = (tally >> 8) & 0x00FF00FFu;   // steps | wins 2 << 16,  wins 1 | draws << 16
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        a += (uint32_t)__shfl_xor((int)a, o);
        b += (uint32_t)__shfl_xor((int)b, o);
    }
    a = __builtin_amdgcn_readfirstlane(a);                             // every lane holds the sums
    b = __builtin_amdgcn_readfirstlane(b);
    n_steps += a & 0xFFFFu;
    n_w2 += a >> 16;
    n_w1 += b & 0xFFFFu;
    n_draw += b >> 16;
    tally = 0u;
}

// The helper: lane l draws for env l of its game wave, from the state words the launch began with and the env's restart
// count alone.  It touches no board and no memory after its two loads (st, rs: the caller's).
// Actions.  Under autoreset every env moves in every step, so step s draws with tick st.w + s; an env that enters the launch
// finished restarts in step 0 without a move and is one tick behind from then on.  Without autoreset a finished env draws
// nothing more, and a live one is at st.w + s as long as it is live.  The bytes are a function of (env, tick0, s).
// Starts.  The game lane reads ordinal nres at its nres-th restart of the launch.  It restarts at most once per step, so with
// c_b its count when block b begins (c_0 = 0, c_b <= c_(b+1) <= c_b + len_b, len_b <= ROLL_R the block's steps) block b reads
// ordinals in (c_b, c_b + len_b] only.  The lane publishes c_b in front of B_b (counts slot b & 1: written before B_b, read by
// the helper after it, and written again only before B_(b+2), which the helper cannot have passed).  The helper carries per
// lane hi, the highest ordinal it has drawn, and TOPS THE RING UP: during block b (behind B_b; behind P for block 0, where
// c_0 = 0 needs no read) it draws (hi, c_b + ROLL_R + len_(b+1)] and sets hi — everything block b + 1 can read, and in
// steady state c_b - c_(b-1) draws: what block b - 1 consumed (2.8 per env and block at 24x24, the slowest lane of a wave
// 4.8, where drawing every block's ROLL_R anew was 8).  The prologue draws (0, len_0]: hi = len_0 at P.  Behind a masked
// entry (roll_resident) the last game_starts = min(ROLL_GAME_STARTS, len_0) of these ordinals are the GAME wave's: the helper
// draws (0, len_0 - game_starts], the game wave (len_0 - game_starts, len_0] with the same make_game_starts (a clash goes
// through make_game_general there as here) into the same slots (episode0 + j) % (2 ROLL_R), both before P; hi = len_0 at P as before.
// The two sets of slots are disjoint (len_0 <= ROLL_R consecutive ordinals), nobody reads the ring before P, and the helper's
// next write is behind P: the invariant below holds with "the ring holds (0, len_0] at P" whoever wrote which slot.
// Invariant: at B_(b+1) the ring holds (c_b, hi] with hi >= c_b + ROLL_R + len_(b+1), which contains block b + 1's (c_(b+1),
// c_(b+1) + len_(b+1)].  Induction: at B_b (P for b = 0) the ring holds (c_(b-1), hi] with hi >= c_(b-1) + ROLL_R + len_b >=
// c_b + len_b (full blocks but the last: hi >= c_b + ROLL_R wherever a block b + 1 exists).  During block b the helper
// writes the ordinals of (hi, c_b + 2 ROLL_R] alone, a subset of (c_b + ROLL_R, c_b + 2 ROLL_R]: not the slots block b
// reads — (c_b, c_b + ROLL_R] and the written set lie in one window of 2 ROLL_R consecutive ordinals — and not the slots
// of (c_b, hi], by the same window; the ordinals those slots held before are 2 ROLL_R lower, at most c_b: consumed.  The
// slot of ordinal j is (episode0 + j) % (2 ROLL_R): episode0 is one constant per lane and launch, so 2 ROLL_R consecutive
// ordinals still fall on 2 ROLL_R different slots and two ordinals share a slot exactly when they are a multiple of
// 2 ROLL_R apart — the window argument concerns consecutive ordinals and is the same as for j % (2 ROLL_R).  A
// count-blind helper (ordinals by block number alone) would need a ring as deep as the launch: an env that has not
// restarted yet still needs ordinal 1 in the last block.  The lanes' counts differ, so the draw loop runs the wave's
// slowest lane's count, the others masked; a clash's general routine runs in it as before, for a third of the draws.
// The last block, a partial one included, reads what was drawn during the block before it (or the prologue), and the
// epilogue's rs4.nstart is the word the lane's last restart read.
// Barriers.  P ends the prologue; B_b opens block b >= 1.  Every wave of the workgroup executes P and B_1 .. B_(nb-1),
// nb = ceil(k_steps / ROLL_R), whatever its role and however many envs it has.  Action block b is written before B_b
// (block 0 before P, block b + 1 during block b, into the slot block b - 1 was read from before B_b — free from the start
// for block 1) and read after it.  The helper draws nothing for a block that will not be played: a launch of one block
// draws block 0 alone, and the last block's starts stop at what its steps can consume.
// TAPE (k_obs_roll_tape, tron_rollout_actions): the action bytes are the caller's.  tape is int8[k_steps][N][2], the launch's
// own first step at row 0, and pass b copies block b + 1's rows of it instead of drawing them: one 2-byte load per env and
// step — the 64 lanes' 128 bytes are contiguous within a step's row —, all of a block's loads in flight at once, each
// player's byte & 3 (what the per-step kernels take from that byte) into bits 0-1 / 2-3 of the ring's byte, where
// draw_action_byte finds x & 3 of a drawn step.  Same slots, same double-buffering, same hand-off at P and B_b; a lane
// without an env of its own (mine false) and a step past k_steps load nothing.  A finished env that restarts in step s
// makes no move in it, as in the per-step kernels: row s is then not used, and nothing is shifted.  The starts ring is
// drawn as ever: a restart's position is keyed by (env, episode), whoever chose the actions.
// Hand-off.  Under autoreset no env is finished when a launch ends and every env has moved in every step, so the launch
// behind this one on the handle — if nobody touches the state words in between, which the host knows (rollout_wave) — starts
// at tick tick0 + k_steps and at episode episode0 + c_final, c_final the env's restarts in this launch.  Its block-0 action
// bytes and its first starts are functions of those and (seed, stream, W, fair) alone, and this helper has nothing to do
// during the last block.  So pass nb - 1 (behind B_(nb-1); behind P in a launch of one block) does not end at once:
//   (a) it tops the start ring up as during any block, as if a block of len_(nb-1) steps followed: it draws
//       (hi, c_(nb-1) + ROLL_R + len_(nb-1)].  The writes obey the window above (at most c_(nb-1) + 2 ROLL_R; in a launch of
//       one block whose prologue drew hi = len_0 < ROLL_R the written (len_0, len_0 + ROLL_R] and the read (0, len_0] lie in
//       (0, 2 ROLL_R]), so the game lane's reads of the last block are undisturbed.  Afterwards the ring holds
//       (c_(nb-1), hi] with hi >= c_(nb-1) + len_(nb-1) + ROLL_R >= c_final + ROLL_R and hi <= c_(nb-1) + 2 ROLL_R <=
//       c_final + 2 ROLL_R: everything in (c_final, c_final + ROLL_R], whatever c_final turns out to be;
//   (b) it draws the next launch's block-0 action bytes, ticks tick0 + k_steps .. + ROLL_R - 1 (TAPE: nothing, the next
//       tape is not known; ROLL_HAND_NO_ACTIONS);
//   (c) it stores the ring's 2 ROLL_R slots as they are in LDS (the slots of consumed ordinals included: nobody reads
//       them), the action qword and episode0 + hi to hand[.][env]: plain stores, nothing waits for them, no barrier.
//       A lane without an env stores nothing.
// Behind a handed entry (ROLL_ENTRY_HANDED) the prologue pass loads these ROLL_HAND_DWORDS words, all loads before the first
// wait, writes the ring and action slot 0, sets hi = word - episode0 (in [ROLL_R, 2 ROLL_R]: "the ring holds (0, hi] at P",
// the invariant's base case with a larger hi) and draws nothing; the game wave draws no start either (game_starts 0).  A
// lane without an env gets hi = 2 ROLL_R, so that it asks for no draw.  Block 0's top-up (hi, ROLL_R + len_1] is then what
// the handed level lacks — nothing for most lanes.  A launch that draws its actions behind a tape launch finds
// ROLL_HAND_NO_ACTIONS and draws block 0's bytes itself; a tape launch copies its rows as ever and takes the starts.
template <bool TAPE>
__device__ __forceinline__ void roll_helper(const Params &P, int env, bool autoreset, const uint4 &st, const uint4 &rs, int k_steps,
                                            int lane, uint2 *aring, uint32_t *sring, const uint32_t *cring, const StepOut &out,
                                            int wave, int gw, bool mine, const int8_t *tape, uint32_t game_starts, uint32_t *hand, bool handed)
{
    ROLL_HSTAMP(0);
    const uint32_t seed = P.seed, stream = P.stream;
    const int W = P.W, fair = P.fair, S = P.S;
    const uint32_t tick0 = st.w - ((autoreset && (st.y & META_DONE)) ? 1u : 0u), ep0 = rs.y;
    const int nb = (k_steps + ROLL_R - 1) / ROLL_R;
    uint32_t *abytes = reinterpret_cast<uint32_t *>(aring);
    uint32_t hi = 0u;                                               // this lane's highest ordinal drawn
    uint32_t *const hme = hand + (mine ? (size_t)env : 0u);         // this env's column of hand[ROLL_HAND_DWORDS][N] (mine only)
    const size_t hn = (size_t)P.N;
    bool have_actions = false;                                      // block 0's bytes came with the hand-off (wave-uniform)
    if (handed) {                                                   // (a launch argument; the host sets it under autoreset alone)
        uint32_t hw[ROLL_HAND_DWORDS];
#pragma unroll
        for (int i = 0; i < ROLL_HAND_DWORDS; ++i) hw[i] = 0u;
        hw[ROLL_HAND_DWORDS - 1] = ep0 + 2u * (uint32_t)ROLL_R;
        if (mine) {
            const uint32_t *q = hme;                                // (the word's address per lane, carried: no offset held in SGPRs)
#pragma unroll
            for (int i = 0; i < ROLL_HAND_DWORDS; ++i, q += hn) hw[i] = *q;   // (all in flight before the first is used)
        }
#pragma unroll
        for (int i = 0; i < 2 * ROLL_R; ++i) sring[i * WAVE + lane] = hw[i];
        hi = hw[ROLL_HAND_DWORDS - 1] - ep0;
        if constexpr (!TAPE) {
            have_actions = __all(hw[2 * ROLL_R + 1] != ROLL_HAND_NO_ACTIONS) != 0;
            if (have_actions) aring[lane] = make_uint2(hw[2 * ROLL_R], hw[2 * ROLL_R + 1]);
        }
    }
    for (int b = -1; b < nb; ++b) {                                 // pass b draws for block b + 1: before P, then during block b
        uint32_t base = 0u;                                         // c_b + ROLL_R: what block b can have consumed at the most
        if (b > 0) {
            ROLL_HSTAMP_BLOCK(b, 0);
            __syncthreads();                                        // B_b
            ROLL_HSTAMP_BLOCK(b, 1);
        }
        const bool last = b + 1 >= nb;                              // the hand-off pass: the launch has no block b + 1
        if (last && !autoreset) break;
        if (b >= 0) base = (b ? cring[(b & 1) * WAVE + lane] : 0u) + (uint32_t)ROLL_R;
        const uint32_t to = base + (uint32_t)min(ROLL_R, k_steps - (last ? b : b + 1) * ROLL_R);
        if (last) {
            // (b) the next launch's block 0, straight to memory
            if constexpr (!TAPE) {
#pragma nounroll
                for (int d = 0; d < ROLL_R / 4; ++d) {
                    uint32_t v = 0u;
#pragma unroll
                    for (uint32_t i = 0; i < 4u; ++i) {
                        uint32_t x[4];
                        philox4x32_10((uint32_t)env, tick0 + (uint32_t)k_steps + (uint32_t)(d * 4) + i, RNG_STEP, 0u, seed, stream, x);
                        v |= action_byte(x[0], x[1]) << (8u * i);
                    }
                    if (mine) hme[(size_t)(2 * ROLL_R + d) * hn] = v;
                }
            } else if (mine) {
                hme[(size_t)(2 * ROLL_R + 1) * hn] = ROLL_HAND_NO_ACTIONS;
            }
        } else if (TAPE || !(b < 0 && have_actions)) {       // (block 0's bytes may have come with the hand-off)
            if constexpr (!TAPE) {
#pragma nounroll
                for (int d = 0; d < ROLL_R / 4; ++d) {                  // four steps' bytes, one dword
                    const uint32_t s0 = (uint32_t)((b + 1) * ROLL_R + d * 4);
                    uint32_t v = 0u;
#pragma unroll
                    for (uint32_t i = 0; i < 4u; ++i) {
                        uint32_t x[4];
                        philox4x32_10((uint32_t)env, tick0 + s0 + i, RNG_STEP, 0u, seed, stream, x);
                        v |= action_byte(x[0], x[1]) << (8u * i);
                    }
                    abytes[(((s0 / ROLL_R) & 1u) * WAVE + (uint32_t)lane) * (ROLL_R / 4) + ((s0 / 4u) & (ROLL_R / 4 - 1))] = v;
                }
            } else {
                const int s0 = (b + 1) * ROLL_R;                        // the block's eight rows: loads first, then the bytes
                const uint16_t *row = reinterpret_cast<const uint16_t *>(tape) + (size_t)s0 * (size_t)P.N + (size_t)env;
                uint32_t t[ROLL_R];
#pragma unroll
                for (int i = 0; i < ROLL_R; ++i) t[i] = (mine && s0 + i < k_steps) ? row[(size_t)i * (size_t)P.N] : 0u;
                uint32_t v[2] = {0u, 0u};
#pragma unroll
                for (int i = 0; i < ROLL_R; ++i) v[i >> 2] |= ((t[i] & 3u) | ((t[i] >> 6) & 0xCu)) << (8 * (i & 3));
                aring[((b + 1) & 1) * WAVE + lane] = make_uint2(v[0], v[1]);
            }
        }
        if (autoreset) {
            const uint32_t upto = b < 0 ? to - min(game_starts, to) : to;   // (block 0's last ordinals may be the game wave's)
#pragma nounroll
            for (uint32_t j = hi + 1u; j <= upto; ++j)              // (per lane: nothing where hi >= upto)
                sring[((ep0 + j) & (2u * ROLL_R - 1u)) * WAVE + (uint32_t)lane] = start_cells_word(S, make_game_starts(seed, stream, W, fair, (uint32_t)env, ep0 + j));
            hi = max(hi, to);
        }
        if (last) {
            // (c) the ring as this lane's own writes (and, in front of P, its game lane's) left it, and its level
            if (mine) {
                uint32_t hw[2 * ROLL_R];
#pragma unroll
                for (int i = 0; i < 2 * ROLL_R; ++i) hw[i] = sring[i * WAVE + lane];
                uint32_t *q = hme;
#pragma unroll
                for (int i = 0; i < 2 * ROLL_R; ++i, q += hn) *q = hw[i];
                q[2u * hn] = ep0 + hi;                              // (behind the two action dwords)
            }
            ROLL_HSTAMP(ROLL_HSTAMPS - 2);
            break;
        }
        if (b < 0) {
            ROLL_HSTAMP(1);
            ROLL_HSTAMP(2);
            __syncthreads();                                        // P
            ROLL_HSTAMP(3);
        }
    }
}

// cell_index for the resident loop's prologue: r + 1 and S are small, one 24-bit multiply-add
__device__ __forceinline__ int roll_cell(int S, int r, int c) { return __mul24(r + 1, S) + (c + 1); }
// One cell of a packed board in LDS, given the board's LDS byte address: memory = (memory & ~mask) | data on the cell's
// dword (lds_cell_dword, lds_cell_shift), the nibble's four bits.  One instruction, nothing read back; a lane's LDS operations execute in order, and the
// memory clobber keeps the compiler's own LDS accesses on their side of it.
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __forceinline__ uint32_t lds_cell_dword(uint32_t board_lds, uint32_t cell) { return board_lds + (cell >> 3) * 4u; }
__device__ __forceinline__ uint32_t lds_cell_shift(uint32_t cell) { return (cell & 7u) * 4u; }
__device__ __forceinline__ void lds_set_nibble(uint32_t dword_lds, uint32_t shift, uint32_t nib)
{
    asm volatile("ds_mskor_b32 %0, %1, %2" : : "v"(dword_lds), "v"(0xFu << shift), "v"(nib << shift) : "memory");
}

template <bool TAPE, bool REC = false>
__device__ __forceinline__ void roll_resident(kernarg_t *kp, int E, int epw, uint32_t cpe, uint32_t flags, const StepOut &out,
                                              int k_steps, unsigned char *smem, const int8_t *tape, unsigned long long *emask, uint32_t *hand)
{
    const uint32_t sd = 2u * cpe + 1u;                              // dwords per board
    uint32_t *boards = reinterpret_cast<uint32_t *>(smem);          // [E][sd]
    uint32_t *tmpl = boards + (size_t)E * sd;                       // [2 cpe] fresh board, packed

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // The workgroup is gw game waves (the low half of the wave indices) and gw helper waves; helper gw + w serves game
    // wave w's envs.  The role is wave-uniform and fixed here.
    const int gw = (int)(blockDim.x >> 7);
    const int hw_wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool helper = hw_wave >= gw;
    const int wave = helper ? hw_wave - gw : hw_wave;               // the game wave (of this wave, or the one this helper serves)
    // per game wave: the store list of up to 64 cpe two-byte entries (the epilogue)
    uint16_t *wlist = reinterpret_cast<uint16_t *>(tmpl + 2u * cpe + (size_t)wave * (32u * cpe));
    // per game wave: the helper's rings (roll_rings) and the restart counts the game lanes publish per block
    uint32_t *rings = tmpl + ((2u * cpe + (size_t)gw * (32u * cpe) + 1u) & ~(size_t)1u) + (size_t)wave * ROLL_RING_DWORDS;
    uint2 *aring = reinterpret_cast<uint2 *>(rings);                // [2][64]: a block's ROLL_R action bytes per env
    uint32_t *sring = rings + 4 * WAVE;                             // [2 ROLL_R][64]: start_cells_word of restart ordinal j in slot (episode0 + j) % (2 ROLL_R)
    uint32_t *cring = sring + 2 * ROLL_R * WAVE;                    // [2][64]: the env's restarts in the launch before block b, in slot b & 1
    // (a tape has no policy: its instantiation holds nothing of TRON_STEP_NONREVERSING)
    const bool autoreset = (flags & TRON_STEP_AUTORESET) != 0u, nonrev = !TAPE && (flags & TRON_STEP_NONREVERSING) != 0u;
    const int we0 = wave * epw;                                     // this wave's first env within the workgroup
    const int e0 = (int)blockIdx.x * E + we0;
    const int env = e0 + lane;
    uint32_t *wboards = boards + (size_t)we0 * sd;
    uint32_t *board = wboards + (size_t)lane * sd;                  // this lane's env
    unsigned char *cellb = reinterpret_cast<unsigned char *>(board);   // two cells per byte
    bool mine;
    int8_t *oenv;                                                   // this env's [2][G] planes
    uint4 st = make_uint4(0u, 0u, 0u, 0u), rs = make_uint4(0u, 0u, 0u, 0u);
    uint2 ab = make_uint2(0u, 0u);                                  // the action bytes of the block being played
    unsigned long long mask = 0ull;                                 // chunks of the player-1 plane that differ from the template
    unsigned long long dirty = 0ull;                                // chunks whose bytes in memory may differ from the board in LDS
    unsigned long long stale = 0ull;                                // chunks that ARE the template, whatever their bytes in LDS say
    bool st_dirty = false;
    uint32_t nres = 0u;                                             // this env's restarts in the launch
    uint32_t n_steps = 0u, n_w1 = 0u, n_w2 = 0u, n_draw = 0u;        // this wave's totals (uniform)
    uint32_t tally = 0u;                                            // this env's share of them, a byte each, since the last flush
    int S = 0;                                                      // all the step loop needs of Params (as S and cell_deltas(S): two SGPRs)

    ROLL_STAMP_LAUNCH(0);
    // ---- prologue: the only loads from memory of the launch
    {
        Params P;
        load_params_scalar(P, kp);
        const int G = P.G;
        S = P.S;
        const int ne = min(min(epw, E - we0), P.N - e0);            // this wave's envs (<= 0: none)
        mine = lane < ne;
        oenv = P.obs_state + (size_t)(mine ? env : 0) * 2u * G;
        const bool masked = (flags & ROLL_ENTRY_MASKED) != 0u;      // (wave-uniform: a launch argument)
        // the ordinals of block 0 that the game wave draws itself behind a masked entry (roll_helper: Starts)
        // (none behind a handed entry: the starts came with the hand-off)
        const bool handed = (flags & ROLL_ENTRY_HANDED) != 0u;
        const uint32_t game_starts = masked && autoreset && !handed ? (uint32_t)min(ROLL_GAME_STARTS, min(ROLL_R, k_steps)) : 0u;
        if (mine) {
            st = P.st4[env];
            if (autoreset) rs = P.rs4[env];
            if (masked && !helper) mask = emask[env];
        }
        for (uint32_t d = (uint32_t)tid; d < 2u * cpe; d += blockDim.x) {
            // eight cells of the fresh board (G % 4 == 0: whole words; a word past G is read as the last one and not used)
            const uint32_t *fw = reinterpret_cast<const uint32_t *>(P.fresh);
            const uint32_t last = (uint32_t)G / 4u - 1u;
            const uint32_t f[2] = {fw[min(2u * d, last)], fw[min(2u * d + 1u, last)]};
            uint32_t v = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j)
                if (d * 8u + j < (uint32_t)G)
                    v |= ((int8_t)(f[j >> 2] >> (8u * (j & 3u))) == TRON_EMPTY ? NIB_EMPTY : NIB_WALL) << (4u * j);
            tmpl[d] = v;
        }
        __syncthreads();
        if (helper) {
            roll_helper<TAPE>(P, env, autoreset, st, rs, k_steps, lane, aring, sring, cring, out, wave, gw, mine, tape, game_starts, hand, handed);
            return;
        }
        if (masked) {
            // ---- the masked entry: the launch before this one left, per env, the mask its epilogue ended with (emask, below) —
            // a superset of the chunks that differ from the template — and stored dirty & (mask | mask0), so memory outside
            // that mask IS the template (a chunk of its mask0 that left its mask went through a restart: dirty, and stored
            // from the template).  Nobody wrote the planes or st4 since (the host's flag behind ROLL_ENTRY_MASKED).  So a
            // chunk outside the mask is entered as stale — the template, whatever its bytes in LDS say: no load, no pack,
            // no LDS write — and only the mask's chunks are read.  mask0 = mask is then a superset of what differs in
            // memory, which is all the epilogue's filter needs; "stale is a subset of dirty" does not hold for the
            // chunks entered stale, and need not: they are the template in memory too, and whoever makes one dirty (a
            // move's refresh, a restart) stores it by the same rules.  A lane without an env has an empty mask.
            // The gather is the epilogue's list run backwards: the same seven-ballot prefix sum, the same wlist region
            // (free until the epilogue), entries (owner lane, chunk); lane l of trip t loads entry 64 t + l, whoever owns
            // it, packs it and writes the two dwords into the owner's board.  The loads of up to GF trips are all issued
            // before the first is waited for: one exposed round trip per GF trips (T is 3.5 per env at 24x24 under random
            // play: four trips).  Lanes write boards they do not own: fence and wave barrier as in the epilogue.
            stale = ~mask & (cpe >= 64u ? ~0ull : (1ull << cpe) - 1ull);
            unsigned long long m = mask;
            const uint32_t cnt = (uint32_t)__popcll(m);
            uint32_t pos = 0u, T = 0u;
#pragma unroll
            for (uint32_t b = 0; b < 7u; ++b) {
                const unsigned long long bm = __ballot(((cnt >> b) & 1u) != 0u);
                pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u)) << b;
                T += (uint32_t)__popcll(bm) << b;
            }
            if (T) {
                for (uint32_t p = pos; m; ++p) {
                    wlist[p] = (uint16_t)(((uint32_t)lane << 6) | ((uint32_t)__ffsll((long long)m) - 1u));
                    m &= m - 1ull;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int8_t *const obase = P.obs_state + (size_t)e0 * 2u * G;     // this wave's first env
                constexpr uint32_t GF = 8u;
                for (uint32_t t0 = 0u; t0 < T; t0 += 64u * GF) {                    // (t0 and T are wave-uniform)
                    uint32_t ent[GF];
                    uint4 v[GF];
#pragma unroll
                    for (uint32_t j = 0; j < GF; ++j) ent[j] = wlist[min(t0 + 64u * j + (uint32_t)lane, T - 1u)];
#pragma unroll
                    for (uint32_t j = 0; j < GF; ++j)                               // (a lane past T reads the last entry's chunk again)
                        if (t0 + 64u * j < T)
                            v[j] = load_chunk<true>(obase + (__umul24(ent[j] >> 6, 2u * (uint32_t)G) + (ent[j] & 63u) * 16u));
#pragma unroll
                    for (uint32_t j = 0; j < GF; ++j)
                        if (t0 + 64u * j < T && t0 + 64u * j + (uint32_t)lane < T) {
                            const uint32_t own = ent[j] >> 6, k = ent[j] & 63u;
                            const int nb = G - (int)k * 16;                         // valid cells of the chunk (G % 4 == 0)
                            if (nb <= 4) v[j].y = 0u;                               // the over-read past G (the player-2 plane) is no board
                            if (nb <= 8) v[j].z = 0u;
                            if (nb <= 12) v[j].w = 0u;
                            uint32_t *b = wboards + __umul24(own, sd) + 2u * k;
                            b[0] = pack_codes8(v[j].x, v[j].y);
                            b[1] = pack_codes8(v[j].z, v[j].w);
                        }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            // the last game_starts ordinals of block 0's (0, len_0], into the slots the helper leaves alone before P
            if (game_starts) {
                const uint32_t to = (uint32_t)min(ROLL_R, k_steps);
#pragma nounroll
                for (uint32_t j = to - game_starts + 1u; j <= to; ++j)
                    sring[((rs.y + j) & (2u * ROLL_R - 1u)) * WAVE + (uint32_t)lane] = start_cells_word(S, make_game_starts(P.seed, P.stream, P.W, P.fair, (uint32_t)env, rs.y + j));
            }
        } else {
            // The wave reads its envs' player-1 planes one env at a time, lane = chunk (coalesced), packs them into the env's
            // board and compares with the template: the ballot is the env's mask.  A plane byte outside the six codes cannot
            // occur in mode None: the planes are written by k_obs_reset and the attach (code1 of a tile value: six codes, the
            // slide tiles' among them), by the moves of obs_tile / k_inc / this kernel (the constants -2, -3, 10, -10) and from
            // the fresh-board template (1 / -1), and the caller never writes the buffer — so the low nibble is the code.
            const bool ck = (uint32_t)lane < cpe;
            const int nb = G - lane * 16;                               // valid cells of this lane's chunk (G % 4 == 0)
            const uint32_t t0 = ck ? tmpl[2 * lane] : 0u, t1 = ck ? tmpl[2 * lane + 1] : 0u;
            // Loads in flight (unconditional, so that they are: a lane or an env past the end reads chunk 0 / the last env again).
            // 16 in flight (95 VGPRs) measured no faster than 8 in either form of the benchmark (profiles/r10_rollout_ab.txt).
            constexpr int PF = 8;
            for (int e = 0; e < ne; e += PF) {
                uint4 v[PF];
#pragma unroll
                for (int j = 0; j < PF; ++j)
                    v[j] = load_chunk<true>(P.obs_state + (size_t)(e0 + min(e + j, ne - 1)) * 2u * G + (ck ? lane * 16 : 0));
#pragma unroll
                for (int j = 0; j < PF; ++j) {
                    if (e + j >= ne) break;
                    uint32_t p0 = 0u, p1 = 0u;
                    if (ck) {
                        if (nb <= 4) v[j].y = 0u;                       // the over-read past G (the player-2 plane) is no board
                        if (nb <= 8) v[j].z = 0u;
                        if (nb <= 12) v[j].w = 0u;
                        p0 = pack_codes8(v[j].x, v[j].y);
                        p1 = pack_codes8(v[j].z, v[j].w);
                        uint32_t *b = wboards + (size_t)(e + j) * sd + 2 * lane;
                        b[0] = p0;
                        b[1] = p1;
                    }
                    const unsigned long long diff = __ballot(ck && (p0 != t0 || p1 != t1));
                    if (lane == e + j) mask = diff;
                }
            }
        }
        ROLL_HSTAMP(ROLL_HSTAMPS - 1);                              // (the game wave's arrival at P, in its helper's region)
        __syncthreads();                                           // the boards and the helpers' block 0 are in LDS before anyone reads them
    }
    const unsigned long long mask0 = mask;                          // chunks that differ from the template IN MEMORY until the epilogue
    // REC: the record tapes' rows of the step being played (wave-uniform; the launch's own first step is row 0)
    size_t row = 0;                                                 // in envs: N per step (no multiply in the loop)

    // ---- the env's state, decoded once: the loop carries these in place of st and the epilogue packs them again
    int cell[2];                                                    // the heads, in cell space (a dead player's may be on the border ring)
    {
        int r[2], c[2];
        unpack_pos(st.x, r, c);
        cell[0] = roll_cell(S, r[0], c[0]);
        cell[1] = roll_cell(S, r[1], c[1]);
    }
    const uint32_t deltas = cell_deltas(S);                         // launch-uniform: one SGPR
    uint32_t alive = st.y & 3u;
    bool done = (st.y & META_DONE) != 0u;
    int winner = (int)((st.y >> 4) & 3u);
    uint32_t last[2] = {(st.y >> 8) & 0xFu, (st.y >> 12) & 0xFu};   // the players' last actions + 1, 0 before a game's first move
    // The heads' chunks of a game in progress are in mask (the invariants above) and a move marks only the NEW heads' chunks;
    // the chunks of the heads the launch begins with are marked dirty here, once.
    if (mine && !done) dirty = (1ull << (cell[0] >> 4)) | (1ull << (cell[1] >> 4));
    uint32_t eplen = st.z, tick = st.w;
    rs.z = start_cells_word(S, rs.z);                               // rs4.nstart in the ring's format (the epilogue converts it back; every lane, a launch without autoreset's zero word too: never read there)
    const uint32_t board_lds = (uint32_t)(uintptr_t)(lds_u32 *)board;
    uint32_t hdw[2] = {lds_cell_dword(board_lds, (uint32_t)cell[0]), lds_cell_dword(board_lds, (uint32_t)cell[1])};   // the heads' dwords in LDS
    uint32_t hsh[2] = {lds_cell_shift((uint32_t)cell[0]), lds_cell_shift((uint32_t)cell[1])};                         // and their nibbles' shifts
    uint32_t snext = (rs.y + 1u) & (2u * ROLL_R - 1u);              // the start ring's slot of episode rs.y + 1: what the next restart reads

    for (int s0 = 0; s0 < k_steps; s0 += ROLL_R) {
        // ---- a block begins.  The one barrier per block: behind it the helper has this block's action bytes and the
        // starts of the restart ordinals up to nres + ROLL_R in the rings, and may overwrite what the block before
        // read; in front of it this lane publishes its restart count for the helper's next draws.
        if (s0) {
            if (out.totals && (s0 & 127) == 0) roll_flush_tally(tally, n_steps, n_w1, n_w2, n_draw);
            cring[((s0 / ROLL_R) & 1) * WAVE + lane] = nres;
            __syncthreads();
        }
        ab = aring[((s0 / ROLL_R) & 1) * WAVE + lane];
        asm volatile("" : "+v"(ab.x), "+v"(ab.y));                  // consumed here, once: the wait for the block's bytes stands in front of the inner loop, not in every step's tail
        const int s1 = min(s0 + ROLL_R, k_steps);
        // The block's steps, once per policy: the launch-uniform flag is a template argument of the body, so the uniform
        // policy's steps hold nothing of the non-reversing draw (its selects were per-step VALU instructions) and the
        // choice is one uniform branch per block.
        auto block_steps = [&](auto nr) __attribute__((always_inline)) {
        constexpr bool NONREV = decltype(nr)::value;
#pragma nounroll
        for (int s = s0; s < s1; ++s) {                             // the block's steps: ab.x's low byte is this step's
            Params P;                                                   // REC alone: N and the reward table, re-read per step (see k_obs_roll)
            if constexpr (REC) load_params_scalar(P, kp);
            ROLL_STAMP(0);

            // ---- the step's one body: the move's judgement, then the board work of the move or of the restart
            const bool stepped = mine && !done;
            // The next game's kit, read speculatively in the step's one LDS round trip, whoever restarts: the template's two
            // dwords of the two start chunks (rs.z has been in registers since the restart before, or the prologue) and the
            // ring's word of the game after it (the slot of episode rs.y + 1: the ordinal nres + 1 <= c_b + len_b of roll_helper's
            // invariant at every step of the block, so the slot is one the helper does not write during this block; a lane
            // that does not restart drops the word, and so does a launch without autoreset, whose ring nobody filled).
            // (scalars, not arrays: a select between two arrays' elements becomes a select of addresses, and the arrays scratch)
            const uint32_t scell_a = rs.z & 0xFFFFu, scell_b = rs.z >> 16;
            uint32_t sk_a = scell_a >> 4, sk_b = scell_b >> 4;
            asm("" : "+v"(sk_a), "+v"(sk_b));                           // (each chunk's two dwords are one ds_read2)
            const uint32_t ts0_a = tmpl[2u * sk_a], ts1_a = tmpl[2u * sk_a + 1u], ts0_b = tmpl[2u * sk_b], ts1_b = tmpl[2u * sk_b + 1u];
            const uint32_t nx = sring[snext * WAVE + (uint32_t)lane];
            float rw0 = 0.0f, rw1 = 0.0f;
            int ncell_a = 0, ncell_b = 0;                               // the new heads: the old ones' cells +-1 or +-S
            uint32_t nk_a = 0u, nk_b = 0u, tc0_a = 0u, tc0_b = 0u, tc1_a = 0u, tc1_b = 0u;
            bool sl_a = false, sl_b = false;
            if (stepped) {
                int ncell[2];
                uint32_t nk[2], tc0[2], tc1[2];
                bool sl[2];
                const uint32_t abyte = ab.x & 0xFFu;
                const int a[2] = {draw_action_byte(abyte, 0, last[0], NONREV), draw_action_byte(abyte, 1, last[1], NONREV)};
                uint32_t ndw[2], nsh[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    ncell[p] = cell[p] + cell_delta(deltas, a[p]);
                    nk[p] = (uint32_t)ncell[p] >> 4;
                    asm("" : "+v"(nk[p]));                           // (the chunk index as one value: its two dwords are one ds_read2 / ds_write2)
                    ndw[p] = lds_cell_dword(board_lds, (uint32_t)ncell[p]);
                    nsh[p] = lds_cell_shift((uint32_t)ncell[p]);
                }
                // The round trip's other reads: the dwords of the two new heads and the template's chunks of theirs.  Only a
                // new head can lie in a stale chunk (the old heads' chunks are in mask); its nibble then comes from the template,
                // which is what the chunk holds once it is refreshed below.  The old heads' cells are not read: they are overwritten.
                uint32_t bw[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    bw[p] = *(lds_u32 *)(uintptr_t)ndw[p];
                    tc0[p] = tmpl[2u * nk[p]];
                    tc1[p] = tmpl[2u * nk[p] + 1u];
                    sl[p] = ((stale >> nk[p]) & 1ull) != 0ull;
                }
                uint32_t tf[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const uint32_t tw = (ncell[p] & 8) ? tc1[p] : tc0[p];
                    tf[p] = ((sl[p] ? tw : bw[p]) >> nsh[p]) & 15u;
                }
                plain_targets(cell, ncell, tf, NIB_P1_BODY, NIB_P2_BODY, NIB_P1_HEAD);
#pragma unroll
                for (int p = 0; p < 2; ++p) alive = collide(alive, p, tf[p] == NIB_EMPTY);   // (cell space: off the board is a border WALL)
                done = settle(alive, ncell, winner);
                if constexpr (REC)
                    if (out.reward) step_rewards(P, done, winner, eplen, rw0, rw1);
                last[0] = (uint32_t)a[0] + 1u;
                last[1] = (uint32_t)a[1] + 1u;
                eplen += 1u;
                tick += 1u;
                st_dirty = true;
                ncell_a = ncell[0], ncell_b = ncell[1];
                nk_a = nk[0], nk_b = nk[1];
                tc0_a = tc0[0], tc0_b = tc0[1], tc1_a = tc1[0], tc1_b = tc1[1];
                sl_a = sl[0], sl_b = sl[1];
            }
            // The kit is consumed here, once, on every path: behind the move's wait (LDS returns in order: nothing is left to
            // wait for), and in front of the board work's writes, so that no wait for it stands behind them in the tail.
            asm volatile("" : : "v"(ts0_a), "v"(ts1_a), "v"(ts0_b), "v"(ts1_b), "v"(nx));
            const bool fin = done;                                      // what the step records: the move's outcome, or that of a
            const int win = winner;                                     // game finished before the step (the restart's tail resets both)
            // A restart (ACKTR.py:307-310) is due in the step the game finishes in, and in a launch's first step for an env
            // that entered finished; only the latter makes no move.  The lane then does the move's board work at the start
            // cells in place of the new heads.
            const bool restart = mine && done && autoreset;
            ROLL_STAMP(1);
            if (stepped || restart) {
                // The board work, one piece of code for both: a chunk that must be refreshed gets the template's two dwords (a
                // new head's stale chunk; a restart's two head chunks, always), THEN the cell writes go on top, in the
                // reference's order: bodies, P1's head, P2's (an out-of-bounds head lands on the border WALL cell; a
                // same-cell head-on leaves P2's head; game.py:90-91 for a restart, which writes no body).  Each cell write
                // is one masked OR on the cell's dword; a lane's LDS operations keep their order, so two heads in one chunk
                // or one dword come out right (the chunk is then written twice with the same template bytes before either
                // nibble is set), and the short last chunk is no special case: its padding nibbles are 0 in the template.
                // A restart's old trail is not wiped: its chunks go stale by the mask as it was (an env that finishes in this
                // step has skipped the move's writes and refreshes: there is no move's board work for it).
                if (restart) {
                    dirty |= mask;
                    stale |= mask;
                    mask = 0ull;
                }
                const int wcell[2] = {restart ? (int)scell_a : ncell_a, restart ? (int)scell_b : ncell_b};
                uint32_t wk[2] = {restart ? sk_a : nk_a, restart ? sk_b : nk_b};
                const uint32_t wd0[2] = {restart ? ts0_a : tc0_a, restart ? ts0_b : tc0_b}, wd1[2] = {restart ? ts1_a : tc1_a, restart ? ts1_b : tc1_b};
                const bool rf[2] = {restart || sl_a, restart || sl_b};
                uint32_t wdw[2], wsh[2];
                unsigned long long nb = 0ull;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    asm("" : "+v"(wk[p]));                           // (the chunk index as one value: its two dwords are one ds_write2)
                    wdw[p] = lds_cell_dword(board_lds, (uint32_t)wcell[p]);
                    wsh[p] = lds_cell_shift((uint32_t)wcell[p]);
                    const unsigned long long wbit = 1ull << wk[p];
                    nb |= wbit;
                    if (rf[p]) {
                        board[2u * wk[p]] = wd0[p];
                        board[2u * wk[p] + 1u] = wd1[p];
                        stale &= ~wbit;
                    }
                }
                if (!restart) {
                    lds_set_nibble(hdw[0], hsh[0], NIB_P1_BODY);
                    lds_set_nibble(hdw[1], hsh[1], NIB_P2_BODY);
                }
                lds_set_nibble(wdw[0], wsh[0], NIB_P1_HEAD);
                lds_set_nibble(wdw[1], wsh[1], NIB_P2_HEAD);
                mask |= nb;                                          // (a move's old heads' chunks are in both already)
                dirty |= nb;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    cell[p] = wcell[p];
                    hdw[p] = wdw[p];
                    hsh[p] = wsh[p];
                }
            }
            // ---- a restart's tail: the state words and the next game.  Nothing here waits for LDS: the word of the game after
            // the one that begins was read above.  The carried state becomes restarted_st4's (the heads are at the start
            // cells already): both alive, no last action, eplen 0.  rs4.episode moves on; rs4.envp and rs4.nenvp stay as the
            // prologue read them until the epilogue (no step of mode None reads them).
            if (restart) {
                alive = META_ALIVE0 | META_ALIVE1;
                done = false;
                winner = 0;
                last[0] = last[1] = 0u;
                eplen = 0u;
                st_dirty = true;
                rs.y += 1u;
                nres += 1u;
                rs.z = nx;                                           // the start cells of game rs.y, drawn by the helper
                snext = (snext + 1u) & (2u * ROLL_R - 1u);
            }
            ROLL_STAMP(2);

            // ---- the records (REC alone: the other instantiations hold no record store and no reward) and the totals
            if constexpr (REC) {
                const uint32_t n = (uint32_t)P.N;                           // a row: N envs
                if (mine) {
                    if (out.done) (out.done + row)[(uint32_t)env] = (int8_t)fin;
                    if (out.winner) (out.winner + row)[(uint32_t)env] = (int8_t)win;
                    if (out.reward) (reinterpret_cast<float2 *>(out.reward) + row)[(uint32_t)env] = make_float2(rw0, rw1);
                }
                row += n;
            }
            // per lane, a byte each: steps, player 1 wins, player 2 wins, draws; summed over the wave at a flush
            if (out.totals && stepped) tally += 1u + (fin ? 1u << ((0x00100818u >> (8 * win)) & 31u) : 0u);   // (draw: byte 3)
            ab.x = (ab.x >> 8) | (ab.y << 24);                          // the next step's byte
            ab.y >>= 8;
            ROLL_STAMP(3);
        }
        };
        if (nonrev) block_steps(std::true_type{});
        else block_steps(std::false_type{});
    }

    ROLL_STAMP_LAUNCH(1);
    // ---- epilogue: both planes of the chunks in dirty, from the boards (every board in LDS is final), the state words, and
    // the wave's totals in one atomic per counter
    {
        Params P;
        load_params_scalar(P, kp);
        const int G = P.G;
        // A touched chunk that is the template again (outside mask) and was the template when the prologue read it (outside
        // mask0) holds the same bytes in memory and in LDS: a restart wiped what the launch itself had drawn there.
        dirty &= mask | mask0;
        // The short last chunk (G % 16 cells: border wall, touched after a head died on it and by the restart that clears
        // it) has its own branch, per lane, with dword stores; the whole chunks go through the wave's list, so their stores
        // are whole 16-byte ones.
        const uint32_t tail = (uint32_t)G & 15u;                                // cells of the last chunk if it is short: 4, 8 or 12
        if (tail && ((dirty >> (cpe - 1u)) & 1ull)) {
            dirty &= ~(1ull << (cpe - 1u));
            const uint32_t k = cpe - 1u, cb = k * 16u;
            const uint32_t *const src = ((stale >> k) & 1ull) ? tmpl : board;      // a stale chunk is stored as the template
            const uint32_t p0 = src[2u * k], p1 = src[2u * k + 1u];
            uint32_t w1[4], w2[4];
            expand_codes8(p0, w1[0], w1[1]);
            expand_codes8(p1, w1[2], w1[3]);
            expand_codes8(swap_nibbles8(p0), w2[0], w2[1]);
            expand_codes8(swap_nibbles8(p1), w2[2], w2[3]);
            uint32_t *q1 = reinterpret_cast<uint32_t *>(oenv + cb), *q2 = reinterpret_cast<uint32_t *>(oenv + G + cb);
            q1[0] = w1[0];                                                       // never past G: the next plane starts there
            q2[0] = w2[0];
            if (tail > 4u) {
                q1[1] = w1[1];
                q2[1] = w2[1];
            }
            if (tail > 8u) {
                q1[2] = w1[2];
                q2[2] = w2[2];
            }
        }
        // The whole chunks go through a wave-wide list, so that the wave runs ceil(T / 64) trips of the expensive body and
        // not its slowest lane's count.  Every lane's place in the list is the prefix sum of the lanes' counts, taken bit by
        // bit from ballots (counts are at most 64: seven bits); the entries are (owner lane, chunk) in ascending order, so
        // neighbouring lanes of a trip mostly hold neighbouring chunks of one env.
        const uint32_t cnt = (uint32_t)__popcll(dirty);
        uint32_t pos = 0u, T = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 7u; ++b) {
            const unsigned long long m = __ballot(((cnt >> b) & 1u) != 0u);
            pos += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) << b;
            T += (uint32_t)__popcll(m) << b;
        }
        if (T) {
            for (uint32_t p = pos; dirty; ++p) {
                const uint32_t k = (uint32_t)__ffsll((long long)dirty) - 1u;
                wlist[p] = (uint16_t)(((uint32_t)(stale >> k) & 1u) << 12 | ((uint32_t)lane << 6) | k);   // bit 12: the source is the template
                dirty &= dirty - 1ull;
            }
            // Lanes read the list and boards that other lanes wrote.  Same-wave LDS operations execute in order; the fence
            // holds the compiler to that order as well.
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            int8_t *const obase = P.obs_state + (size_t)e0 * 2u * G;           // this wave's first env
            // An entry is read one trip ahead of the board read that depends on it.
            uint32_t idx = (uint32_t)lane;
            uint32_t ent = wlist[min(idx, T - 1u)];
            while (idx < T) {
                const uint32_t own = (ent >> 6) & 63u, k = ent & 63u;
                const uint32_t *const ob = ((ent >> 12) ? tmpl : wboards + __umul24(own, sd)) + 2u * k;   // the owner's board, or the template for a stale chunk
                const uint32_t p0 = ob[0], p1 = ob[1];
                idx += 64u;
                ent = wlist[min(idx, T - 1u)];
                uint32_t w1[4], w2[4];
                expand_codes8(p0, w1[0], w1[1]);
                expand_codes8(p1, w1[2], w1[3]);
                expand_codes8(swap_nibbles8(p0), w2[0], w2[1]);
                expand_codes8(swap_nibbles8(p1), w2[2], w2[3]);
                int8_t *const q = obase + (__umul24(own, 2u * (uint32_t)G) + k * 16u);
                *reinterpret_cast<U4A4 *>(q) = U4A4{w1[0], w1[1], w1[2], w1[3]};
                *reinterpret_cast<U4A4 *>(q + G) = U4A4{w2[0], w2[1], w2[2], w2[3]};
            }
        }
        ROLL_STAMP_LAUNCH(2);
        // st4 is packed here alone, from the carried state: the bytes stepped_st4 or restarted_st4 of the env's last event
        // would have left (last[] is the stored action + 1, and 0 behind a restart; a dead player's head may be off the board)
        // r and c come back from the cells (cells_pos: one division by S per env and launch) — a dead player's head on the
        // border ring gives the -1 or W that carrying r and c through the moves gave
        if (mine && st_dirty) {
            P.st4[env] = make_uint4(cells_pos(S, cell[0], cell[1]), pack_meta(alive, done, winner, (int)last[0] - 1, (int)last[1] - 1), eplen, tick);
        }
        // The next launch's entry mask (the masked entry above): what differs from the template now lies inside mask, and the
        // stores above left memory outside it the template.  Every env of the launch, a lane that did not step (the mask it
        // entered with) included.
        if (mine) emask[env] = mask;
        // rs4.envp / rs4.nenvp of an env that restarted, drawn here once instead of at every restart: nenvp belongs to the
        // game at the final `episode`; envp is what nenvp was before the env's last restart — the word the prologue read
        // after one restart (so what tron_set_weight_degree put into envp leaves with the first restart, as it always
        // did), the game at episode - 1 after two and more.  The full make_game, clash path included.
        if (mine && nres) {
            uint32_t envp = rs.w;
#pragma nounroll
            for (uint32_t back = min(nres, 2u) - 1u; (int)back >= 0; --back) {
                const NewGame ng = make_game(P.seed, P.stream, P.W, P.fair, (uint32_t)env, rs.y - back);
                if (back) envp = pack_envp(ng.w0, ng.w1, ng.degree);
                else rs.w = pack_envp(ng.w0, ng.w1, ng.degree);
            }
            rs.x = envp;
            rs.z = cells_pos(S, (int)(rs.z & 0xFFFFu), (int)(rs.z >> 16));   // the ring's word back to pack_pos (a lane that never restarted stores nothing)
            P.rs4[env] = rs;
        }
    }
    ROLL_STAMP_LAUNCH(3);
#ifndef TRON_STAMPS
    if (out.totals) roll_flush_tally(tally, n_steps, n_w1, n_w2, n_draw);
    if (out.totals && lane == 0) {
        if (n_steps) atomicAdd(&out.totals[0], (unsigned long long)n_steps);
        if (n_w1) atomicAdd(&out.totals[1], (unsigned long long)n_w1);
        if (n_w2) atomicAdd(&out.totals[2], (unsigned long long)n_w2);
        if (n_draw) atomicAdd(&out.totals[3], (unsigned long long)n_draw);
    }
#endif
}

// The random-action rollout as ONE launch for k_steps steps (tron_rollout_random): envs never interact, so a wave can
// step its own envs k_steps times without waiting for anybody else — there is no drain of the whole chip between steps
// and no barrier between the waves of a workgroup.  The same results, bit for bit, as k_steps launches of k_obs, in memory
// when the launch ends: the planes and the state words are written by its epilogue, not by its steps.
// E envs per workgroup, epw (<= 64) per wave, blockDim.x / 64 waves; gridDim.x == ceil(N / E).  Mode None, int8 codes,
// even side, cpe <= 64 (roll_resident).  TRON_ROLLOUT_RESIDENT asks for what this kernel does by itself; the flag is
// accepted for its callers' sake.
__global__ __launch_bounds__(2 * BLOCK) void k_obs_roll(Params P, int E, int epw, uint32_t cpe, uint32_t flags, StepOut out, int k_steps,
                                                        unsigned long long *__restrict__ emask, uint32_t *__restrict__ hand)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // Params is read from the kernel-argument segment where it is needed (scalar loads through a pointer the compiler
    // cannot see through: the prologue, the epilogue, REC's steps) instead of kept live across the loop: 26 words of
    // Params in SGPRs for the whole launch spill, and every spilled word is a v_readlane per use.  S and W do stay live.
    kernarg_t *kp = (kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr();       // (Params is the first argument)
    roll_resident<false>(kp, E, epw, cpe, flags & ~TRON_ROLLOUT_RESIDENT, out, k_steps, smem, nullptr, emask, hand);
}

// The same launch with the caller's actions (tron_rollout_actions): the second instantiation of roll_resident.  Its game
// waves run k_obs_roll's loop on bytes of the same ring; only its helper differs (roll_helper<true>), and tape points at the
// launch's own first step.
__global__ __launch_bounds__(2 * BLOCK) void k_obs_roll_tape(Params P, int E, int epw, uint32_t cpe, uint32_t flags, StepOut out, int k_steps,
                                                             const int8_t *__restrict__ tape, unsigned long long *__restrict__ emask, uint32_t *__restrict__ hand)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    kernarg_t *kp = (kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr();       // (Params is the first argument: see k_obs_roll)
    roll_resident<true>(kp, E, epw, cpe, flags, out, k_steps, smem, tape, emask, hand);
}

// k_obs_roll_tape with the per-step records (tron_rollout_actions_records): the third instantiation of roll_resident.  Same
// step loop, same helper; out.done / out.winner / out.reward are step-major tapes here and point, like tape, at the launch's
// own first step.
__global__ __launch_bounds__(2 * BLOCK) void k_obs_roll_tape_rec(Params P, int E, int epw, uint32_t cpe, uint32_t flags, StepOut out, int k_steps,
                                                                 const int8_t *__restrict__ tape, unsigned long long *__restrict__ emask, uint32_t *__restrict__ hand)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    kernarg_t *kp = (kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr();       // (Params is the first argument: see k_obs_roll)
    roll_resident<true, true>(kp, E, epw, cpe, flags, out, k_steps, smem, tape, emask, hand);
}

// Fewer workgroups than tiles (the TRON_ROLL_GRID override): workgroup w owns tiles w, w + gridDim.x, ... and
// every step reads its tile's state from memory and rewrites both planes (obs_tile, as k_obs).  Every
// workgroup runs a fixed trip count, so the grid always drains.
__global__ __launch_bounds__(BLOCK) void k_obs_roll_walk(Params P, int E, uint32_t cpe, uint32_t cpe_magic, uint32_t flags,
                                                        StepOut out, int k_steps, int ntiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long acc[4];           // see k_obs_roll
    StepOut lo = out;
    if (out.totals) {
        if (threadIdx.x < 4) acc[threadIdx.x] = 0ull;
        lo.totals = acc;
        __syncthreads();
    }
    flags &= ~TRON_ROLLOUT_RESIDENT;
    kernarg_t *kp = (kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr();       // (Params is the first argument: see k_obs_roll)
    for (int s = 0; s < k_steps; ++s)
        for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
            kernarg_t *q = kp;
            asm volatile("" : "+s"(q));
            Params Pl;
            load_params(Pl, q);
            obs_tile<true>(Pl, E, cpe, cpe_magic, nullptr, flags, lo, t, smem);
            __syncthreads();        // the tile's LDS is reused; this step's state words are visible to the next
        }
    if (out.totals && threadIdx.x < 4 && acc[threadIdx.x]) atomicAdd(&out.totals[threadIdx.x], acc[threadIdx.x]);
}

// load_params reads sizeof(Params) bytes from offset 0 of the kernel-argument segment: that is Params only while it is the
// kernel's FIRST parameter (arguments are laid out in declaration order from offset 0) and a plain block of bytes.
template <class F> struct first_kernel_arg;
template <class R, class A0, class... A> struct first_kernel_arg<R (*)(A0, A...)> { typedef A0 type; };
static_assert(std::is_same<first_kernel_arg<decltype(&k_obs_roll)>::type, Params>::value,
              "k_obs_roll re-reads Params from kernarg offset 0: Params must stay its first parameter");
static_assert(std::is_same<first_kernel_arg<decltype(&k_obs_roll_walk)>::type, Params>::value, "k_obs_roll_walk re-reads Params from kernarg offset 0");
static_assert(std::is_same<first_kernel_arg<decltype(&k_obs_roll_tape)>::type, Params>::value, "k_obs_roll_tape re-reads Params from kernarg offset 0");
static_assert(std::is_same<first_kernel_arg<decltype(&k_obs_roll_tape_rec)>::type, Params>::value, "k_obs_roll_tape_rec re-reads Params from kernarg offset 0");
static_assert(std::is_trivially_copyable<Params>::value && alignof(Params) <= 8 && sizeof(Params) % 4 == 0,
              "Params is block-copied from the kernel-argument segment with scalar loads");

// the sliding modes' persistent rollout: k_obs_roll's loop on obs_tile<true, true>
#ifndef TRON_SLIDE_KERNARG_REREAD
#define TRON_SLIDE_KERNARG_REREAD 1   // as k_obs_roll: Params re-read from the kernel-argument segment per step (69 -> 41 SGPR spills; temper 0.750 -> 0.757, 0.720 -> 0.734 at 20 steps per launch)
#endif
__global__ __launch_bounds__(BLOCK) void k_obs_roll_slide(Params P, int E, uint32_t cpe, uint32_t cpe_magic, uint32_t flags,
                                                         StepOut out, int k_steps, int ntiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long acc[4];           // see k_obs_roll
    StepOut lo = out;
    if (out.totals) {
        if (threadIdx.x < 4) acc[threadIdx.x] = 0ull;
        lo.totals = acc;
        __syncthreads();
    }
    const bool resident = (flags & TRON_ROLLOUT_RESIDENT) != 0u && (int)gridDim.x == ntiles;
    flags &= ~TRON_ROLLOUT_RESIDENT;
#if TRON_SLIDE_KERNARG_REREAD
    kernarg_t *kp = (kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr();       // (Params is the first argument: see k_obs_roll)
#endif
    for (int s = 0; s < k_steps; ++s)
        for (int t = (int)blockIdx.x; t < ntiles; t += (int)gridDim.x) {
#if TRON_SLIDE_KERNARG_REREAD
            kernarg_t *q = kp;
            asm volatile("" : "+s"(q));
            Params Pl;
            load_params(Pl, q);
            obs_tile<true, true>(Pl, E, cpe, cpe_magic, nullptr, flags, lo, t, smem, resident && s > 0, resident);
#else
            obs_tile<true, true>(P, E, cpe, cpe_magic, nullptr, flags, lo, t, smem, resident && s > 0, resident);
#endif
            __syncthreads();
        }
    if (out.totals && threadIdx.x < 4 && acc[threadIdx.x]) atomicAdd(&out.totals[threadIdx.x], acc[threadIdx.x]);
}
static_assert(std::is_same<first_kernel_arg<decltype(&k_obs_roll_slide)>::type, Params>::value, "k_obs_roll_slide may re-read Params from kernarg offset 0");

// ------------------------------------------------------------ incremental step --
// Observation-is-state, TRON_STEP_INCREMENTAL: the attached planes already hold the previous
// observation, and a move changes at most 4 cells per plane, so only those cells are written;
// only boards that restart are rewritten in full.  No tile, no LDS staging: ONE ENV PER LANE
// (wave 0 of each 64-env workgroup) reads its state words and two target cells, decides, and
// stores 8 bytes; the four waves then share the rewrites of the restarting boards (coalesced
// 16-byte stores from an LDS template).
// HBM traffic per env-step is ~100 B + 2G per restart instead of 3G — this is a different
// contract from "both planes written every step" and is reported under its own label.
template <int DUMMY>
__global__ __launch_bounds__(BLOCK) void k_inc(Params P, uint32_t cpe, const int8_t *__restrict__ actions,
                                               uint32_t flags, StepOut out)
{
    // 256 threads per 64 envs: wave 0 decides (lane = env), wave 1 draws the speculative next start,
    // then all four waves share the rewrites of the restarting boards.
    __shared__ uint4 tmpl[640];                                   // fresh board as codes (same for both players)
    __shared__ uint4 rec_rs[WAVE];                                // new rs4 of an env, should it restart
    __shared__ uint32_t rec_nstart[WAVE];                         // its cached start positions (rs4.z)
    __shared__ uint32_t rec_heads[WAVE];                          // restart word (restart_word)
    const int G = P.G, S = P.S, W = P.W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int env = blockIdx.x * WAVE + lane;
    const bool mine = env < P.N;
    const bool autoreset = (flags & TRON_STEP_AUTORESET) != 0u, nonrev = (flags & TRON_STEP_NONREVERSING) != 0u;

    uint4 st = make_uint4(0u, META_DONE, 0u, 0u), rs = make_uint4(0u, 0u, 0u, 0u);
    uint32_t act = 0u;
    if (mine && wave == 0) {
        st = P.st4[env];
        if (actions) act = reinterpret_cast<const uint16_t *>(actions)[env];
    }
    if (mine && wave == 1 && autoreset) rs = P.rs4[env];
    if (autoreset)
        for (uint32_t d = (uint32_t)tid; d < cpe * 16u; d += BLOCK)
            reinterpret_cast<int8_t *>(tmpl)[d] = (d < (uint32_t)G) ? (P.fresh[d] == TRON_EMPTY ? (int8_t)1 : (int8_t)-1) : (int8_t)0;
    if (wave == 1 && autoreset) {
        rec_nstart[lane] = rs.z;
        if (mine) {
            const NewGame ng = make_game(P.seed, P.stream, W, P.fair, (uint32_t)env, rs.y + 1u);
            rec_rs[lane] = make_uint4(rs.w, rs.y + 1u, pack_pos(ng.r1, ng.c1, ng.r2, ng.c2), pack_envp(ng.w0, ng.w1, ng.degree));
        }
    }

    bool restart = false, done = false, stepped = false;
    int winner = 0;
    uint4 new_st = st;
    if (wave == 0) {
        int8_t *o1 = P.obs_state + (size_t)(mine ? env : 0) * 2u * G, *o2 = o1 + G;
        typedef CodeCells C;
        uint32_t m = st.y;
        int r[2], c[2];
        unpack_pos(st.x, r, c);
        done = (m & META_DONE) != 0;
        stepped = mine && !done;
        winner = (int)((m >> 4) & 3u);
        float rw0 = 0.0f, rw1 = 0.0f;
        if (stepped) {
            int a[2];
            if (!actions) {
                uint32_t x[4];
                philox4x32_10((uint32_t)env, st.w, RNG_STEP, 0u, P.seed, P.stream, x);
                a[0] = draw_action(x[0], (m >> 8) & 0xFu, nonrev);
                a[1] = draw_action(x[1], (m >> 12) & 0xFu, nonrev);
            } else {
                a[0] = (int)(act & 3u);
                a[1] = (int)((act >> 8) & 3u);
            }
            // the move of lane_move_codes, its two target cells read from the player-1 plane in memory
            int old[2], f[2], tf[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                int dr, dc;
                action_delta(a[p], dr, dc);
                old[p] = cell_index(S, r[p], c[p]);
                r[p] += dr;
                c[p] += dc;
                f[p] = cell_index(S, r[p], c[p]);
            }
            tf[0] = o1[f[0]];
            tf[1] = o1[f[1]];
            plain_targets(old, f, tf, (int)C::P1_BODY, (int)C::P2_BODY, (int)C::P1_HEAD);
            uint32_t alive = m & 3u;
#pragma unroll
            for (int p = 0; p < 2; ++p) alive = collide(alive, p, W, r[p], c[p], tf[p] == C::EMPTY);
            done = settle(alive, r, c, winner);
            step_rewards(P, done, winner, st.z, rw0, rw1);
            new_st = stepped_st4(r, c, pack_meta(alive, done, winner, a[0], a[1]), st.z, st.w);
            if (!(done && autoreset)) {
                // the four cells, reference order: bodies, P1's head, P2's head — in both planes (the player-2 plane
                // holds the other player's code)
                o1[old[0]] = C::P1_BODY; o2[old[0]] = C::P2_BODY;
                o1[old[1]] = C::P2_BODY; o2[old[1]] = C::P1_BODY;
                o1[f[0]] = C::P1_HEAD;   o2[f[0]] = C::P2_HEAD;
                o1[f[1]] = C::P2_HEAD;   o2[f[1]] = C::P1_HEAD;
                P.st4[env] = new_st;
            }
        }
        if (mine) {
            if (out.done) out.done[env] = (int8_t)done;
            if (out.winner) out.winner[env] = (int8_t)winner;
            if (out.reward) reinterpret_cast<float2 *>(out.reward)[env] = make_float2(rw0, rw1);
        }
        if (out.totals) {
            const int wn = (stepped && done) ? winner : -1;
            const unsigned long long bs = __ballot(stepped);
            const unsigned long long b1 = __ballot(wn == 1), b2 = __ballot(wn == 2), b0 = __ballot(wn == 0);
            if (lane == 0) {
                if (bs) atomicAdd(&out.totals[0], (unsigned long long)__popcll(bs));
                if (b1) atomicAdd(&out.totals[1], (unsigned long long)__popcll(b1));
                if (b2) atomicAdd(&out.totals[2], (unsigned long long)__popcll(b2));
                if (b0) atomicAdd(&out.totals[3], (unsigned long long)__popcll(b0));
            }
        }
        restart = mine && done && autoreset;
    }
    __syncthreads();                                                 // template, rec_rs, rec_nstart are in LDS
    if (wave == 0) {
        uint32_t hw = 0u;
        if (restart) {                                               // ACKTR.py:307-310; start cached one restart ago
            const uint32_t ns = rec_nstart[lane];
            P.st4[env] = restarted_st4(ns, new_st.w);
            P.rs4[env] = rec_rs[lane];
            hw = restart_word(S, ns);
        }
        rec_heads[lane] = hw;
    }
    if (!autoreset) return;
    __syncthreads();

    // ---- restarting boards: both planes from the template, dealt round-robin to the four waves
    const uint32_t my_hw = rec_heads[lane];
    unsigned long long rmask = __ballot(is_restart(my_hw));
    int nth = 0;
    while (rmask) {
        const int e = __ffsll((long long)rmask) - 1;
        rmask &= rmask - 1;
        if ((nth++ & 3) != wave) continue;
        const uint32_t hw = rec_heads[e];
        const uint32_t a1 = restart_head(hw, 0), a2 = restart_head(hw, 1);
        int8_t *q = P.obs_state + (size_t)(blockIdx.x * WAVE + e) * 2u * G;
        for (uint32_t j = (uint32_t)lane; j < 2u * cpe; j += WAVE) {      // chunk k of plane pl
            const uint32_t pl = j >= cpe ? 1u : 0u, k = j - pl * cpe, cc = k * 16u;
            uint4 t = tmpl[k];
            const uint32_t d1 = a1 - cc, d2 = a2 - cc;
            // template head cells are EMPTY (1): XOR to own head 10 / enemy head -10 per plane (game.py:90-91)
            const uint32_t x1 = (uint32_t)(0x01 ^ (pl ? 0xF6 : 0x0A)) << ((d1 & 3u) * 8u);
            const uint32_t x2 = (uint32_t)(0x01 ^ (pl ? 0x0A : 0xF6)) << ((d2 & 3u) * 8u);
            t.x ^= (d1 < 4u ? x1 : 0u) ^ (d2 < 4u ? x2 : 0u);
            t.y ^= (d1 - 4u < 4u ? x1 : 0u) ^ (d2 - 4u < 4u ? x2 : 0u);
            t.z ^= (d1 - 8u < 4u ? x1 : 0u) ^ (d2 - 8u < 4u ? x2 : 0u);
            t.w ^= (d1 - 12u < 4u ? x1 : 0u) ^ (d2 - 12u < 4u ? x2 : 0u);
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
            store_chunk<true>(q + (size_t)pl * G + cc, min(16, G - (int)cc), w);
        }
    }
}

// observation-is-state helpers: board images / other formats from the attached planes
__global__ void k_obs_to_grid(Params P, int8_t *__restrict__ grid_out)
{
    const size_t total = (size_t)P.N * P.G;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t e = i / (size_t)P.G, cidx = i - e * (size_t)P.G;
        grid_out[i] = tile_of_code(P.obs_state[e * 2u * P.G + cidx]);
    }
}
// ... and the slide tiles (sliding modes): a logged cell that still holds its player's body code is that player's slide tile
__global__ void k_obs_grid_marks(Params P, int8_t *__restrict__ grid_out)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= P.N) return;
    const uint32_t cnt = (P.st4[env].y >> SLIDE_CNT_SHIFT) & SLIDE_CNT_MASK;
    const uint16_t *lg = slide_log(P) + (size_t)env * slide_log_len(P.W);
    const int8_t *o = P.obs_state + (size_t)env * 2u * P.G;
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t e = lg[k], cell = e & 0x7FFFu, pl = e >> 15;
        if (o[cell] == (pl ? (int8_t)-3 : (int8_t)-2)) grid_out[(size_t)env * P.G + cell] = pl ? TRON_P2_SLIDE : TRON_P1_SLIDE;
    }
}
// attaching to boards that already hold slide tiles (steps were made on the board-owning layout): their log, from the grid
__global__ void k_obs_attach_marks(Params P)
{
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= P.N) return;
    const int8_t *g = P.grid + (size_t)env * P.G;
    uint16_t *lg = slide_log(P) + (size_t)env * slide_log_len(P.W);
    uint32_t cnt = 0u;
    for (int i = 0; i < P.G; ++i) {
        const int8_t t = g[i];
        if (t == TRON_P1_SLIDE || t == TRON_P2_SLIDE) lg[cnt++] = (uint16_t)((uint32_t)i | (t == TRON_P2_SLIDE ? 0x8000u : 0u));
    }
    uint4 st = P.st4[env];
    st.y = (st.y & ~(SLIDE_CNT_MASK << SLIDE_CNT_SHIFT)) | (cnt << SLIDE_CNT_SHIFT);
    P.st4[env] = st;
}
__global__ void k_obs_reset(Params P, const int8_t *__restrict__ mask)
{
    // after k_reset wrote P.grid for the masked envs: re-derive their two planes from it
    const int env = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (env >= P.N) return;
    if (mask && !mask[env]) return;
    const int8_t *g = P.grid + (size_t)env * P.G;
    int8_t *o = P.obs_state + (size_t)env * 2u * P.G;
    for (int i = lane; i < P.G; i += 64) {
        o[i] = code1(g[i], false);
        o[P.G + i] = code1(g[i], true);
    }
}
// planes (util.pop_up [+ prob_map plane]) of every env from the attached code planes
__global__ void k_obs_planes(Params P, int channels, float *__restrict__ out)
{
    const size_t cells = (size_t)P.G, total = (size_t)P.N * 2u * cells;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t k = i / cells, cidx = i - k * cells;          // k = env*2 + player
        const int v = P.obs_state[i];
        float *o = out + k * (size_t)channels * cells + cidx;
        o[0] = (v == -1) ? 1.0f : 0.0f;
        o[cells] = (v == -2) ? 1.0f : (v == 10) ? 10.0f : 0.0f;
        o[2 * cells] = (v == -3) ? 1.0f : (v == -10) ? 10.0f : 0.0f;
        if (channels == 4) o[3 * cells] = (float)degree_slide(P.slide[k >> 1]);
    }
}

// ------------------------------------------------------------- small kernels --
// make_game / Game.__init__ for masked envs: one wave per env.
__global__ __launch_bounds__(BLOCK) void k_reset(Params P, const int8_t *__restrict__ mask,
                                                 const int8_t *__restrict__ start, const int16_t *__restrict__ weight,
                                                 const int16_t *__restrict__ degree)
{
    const int env = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (env >= P.N) return;
    if (mask && !mask[env]) return;
    const uint32_t epi = P.rs4[env].y;
    NewGame ng;
    if (start) {
        ng.r1 = start[4 * env]; ng.c1 = start[4 * env + 1]; ng.r2 = start[4 * env + 2]; ng.c2 = start[4 * env + 3];
        uint32_t x[4];
        philox4x32_10((uint32_t)env, epi, RNG_INIT, 0u, P.seed, P.stream, x);
        ng.w0 = randint_u32(x[0], 40, 101);                              // game.py:83
        ng.w1 = randint_u32(x[1], 40, 101);
        ng.degree = randint_u32(x[2], -30, 30);                          // game.py:87
    } else {
        ng = make_game(P.seed, P.stream, P.W, P.fair, (uint32_t)env, epi);
    }
    if (weight) { ng.w0 = weight[2 * env]; ng.w1 = weight[2 * env + 1]; }
    if (degree) ng.degree = degree[env];
    const int h1 = cell_index(P.S, ng.r1, ng.c1), h2 = cell_index(P.S, ng.r2, ng.c2);
    int8_t *g = P.grid + (size_t)env * P.G;
    for (int i = lane; i < P.G; i += 64) {
        int8_t v = P.fresh[i];
        if (i == h1) v = TRON_P1_HEAD;                                   // game.py:90-91, pps order
        if (i == h2) v = TRON_P2_HEAD;
        g[i] = v;
    }
    if (lane == 0) {
        const uint32_t tick = P.st4[env].w;
        P.st4[env] = make_uint4(pack_pos(ng.r1, ng.c1, ng.r2, ng.c2), META_ALIVE0 | META_ALIVE1, 0u, tick);
        const NewGame nx = make_game(P.seed, P.stream, P.W, P.fair, (uint32_t)env, epi + 1u);   // the next autoreset's game
        P.rs4[env] = make_uint4(pack_envp(ng.w0, ng.w1, ng.degree), epi + 1u, pack_pos(nx.r1, nx.c1, nx.r2, nx.c2),
                                pack_envp(nx.w0, nx.w1, nx.degree));
    }
}

__global__ void k_fresh(int8_t *fresh, int S)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * S) return;
    const int r = i / S, c = i - r * S;
    fresh[i] = (r == 0 || r == S - 1 || c == 0 || c == S - 1) ? TRON_WALL : TRON_EMPTY;   // map.py:5-6,48
}

__global__ void k_fill_f64(double *dst, double v, const double *src, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src ? src[i] : v;
}

__global__ void k_set_wd(Params P, const int16_t *weight, const int16_t *degree)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    uint32_t ep = P.rs4[i].x;
    if (weight) ep = (ep & 0xFFFF0000u) | (uint32_t)(uint8_t)weight[2 * i] | ((uint32_t)(uint8_t)weight[2 * i + 1] << 8);
    if (degree) ep = (ep & 0xFF00FFFFu) | ((uint32_t)(uint8_t)(int8_t)degree[i] << 16);
    P.rs4[i].x = ep;
}

__global__ void k_copy16(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n16, const int8_t *src8,
                         int8_t *dst8, size_t nbytes)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
    if (blockIdx.x == 0)
        for (size_t b = n16 * 16 + threadIdx.x; b < nbytes; b += blockDim.x) dst8[b] = src8[b];
}

__global__ void k_get_state(Params P, int8_t *pos, int8_t *alive, int8_t *dir, int8_t *done, int8_t *winner,
                            int16_t *weight, int16_t *degree, double *slide, uint32_t *counters)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.N) return;
    const uint4 st = P.st4[i], rs = P.rs4[i];
    const uint32_t pw = st.x, m = st.y, ep = rs.x;
    if (pos) reinterpret_cast<uint32_t *>(pos)[i] = pw;
    if (alive) { alive[2 * i] = (int8_t)(m & 1u); alive[2 * i + 1] = (int8_t)((m >> 1) & 1u); }
    if (dir) { dir[2 * i] = (int8_t)((m >> 8) & 7u); dir[2 * i + 1] = (int8_t)((m >> 12) & 7u); }
    if (done) done[i] = (int8_t)((m >> 2) & 1u);
    if (winner) winner[i] = (int8_t)((m >> 4) & 3u);
    if (weight) { weight[2 * i] = (int16_t)(ep & 0xFFu); weight[2 * i + 1] = (int16_t)((ep >> 8) & 0xFFu); }
    if (degree) degree[i] = (int16_t)(int8_t)(ep >> 16);
    if (slide) slide[i] = P.slide[i];
    if (counters) { counters[3 * i] = st.w; counters[3 * i + 1] = rs.y; counters[3 * i + 2] = st.z; }
}

// Map.state_for_player on arbitrary tile images (map.py:67-84)
__global__ void k_encode_codes(const int8_t *__restrict__ tiles, size_t nbytes, int player_is_2, int8_t *__restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x * 16;
    for (size_t b = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; b < nbytes; b += stride) {
        if (b + 16 <= nbytes) {
            const uint4 t = *reinterpret_cast<const uint4 *>(tiles + b);
            *reinterpret_cast<uint4 *>(out + b) = make_uint4(codes4(t.x, player_is_2), codes4(t.y, player_is_2),
                                                             codes4(t.z, player_is_2), codes4(t.w, player_is_2));
        } else {
            for (size_t j = b; j < nbytes; ++j) out[j] = code1(tiles[j], player_is_2);
        }
    }
}

// util.pop_up on code planes (util.py:11-37): (wall, my, enemy)
__global__ void k_pop_up(const int8_t *__restrict__ codes, size_t n, int cells, float *__restrict__ out)
{
    const size_t total = n * (size_t)cells;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t k = i / (size_t)cells, cidx = i - k * (size_t)cells;
        const int v = codes[i];
        float *o = out + k * 3 * (size_t)cells + cidx;
        o[0] = (v == -1) ? 1.0f : 0.0f;
        o[cells] = (v == -2) ? 1.0f : (v == 10) ? 10.0f : 0.0f;
        o[2 * (size_t)cells] = (v == -3) ? 1.0f : (v == -10) ? 10.0f : 0.0f;
    }
}

}  // namespace

// ---------------------------------------------------------------- host side --
struct tron_env {
    Params P;
    int device;
    int E;                    // envs per workgroup tile
    uint32_t cpe, cpe_magic;  // 16-byte chunks per env, ceil(2^32 / cpe)
    size_t smem;              // dynamic LDS bytes
    bool aligned;             // G % 4 == 0: 16-byte global accesses
    void *blob;               // one allocation behind all state arrays
    hipStream_t side;         // TRON_ROLLOUT_TWO_STREAMS: second launch stream + fork/join events, created on first use
    hipEvent_t fork, join;
    int part0, nparts;        // slice of the tiles the next launch covers (0, 1 = all of them)
    int roll_E;               // envs per tile of the persistent rollout (0: not chosen yet), see roll_tile_envs
    int roll_waves;           // waves per workgroup of k_obs_roll (0: not chosen yet), see roll_waves
    unsigned long long *emask; // [N] in the blob: k_obs_roll's entry masks, written by every launch of the roll_resident family
    uint32_t *hand;           // [ROLL_HAND_DWORDS][N] in the blob, next to the entry masks: the helper's hand-off (roll_helper)
    bool entry_masks;         // the entry masks describe the attached planes: the last call that could write the planes or the
                              // state words enqueued was such a launch over all envs (set in rollout_wave, cleared by launch()
                              // per writes_state; it follows the order of the calls, as the planes follow the order of the stream)
    bool handed;              // `hand` is what the next launch of the family would draw: the last call enqueued that could write
                              // the state words was such a launch with autoreset, made with the four values below (set in
                              // rollout_wave, cleared like entry_masks and by a launch without autoreset)
    uint32_t hand_seed, hand_stream;
    int hand_fair, hand_W;
};

namespace {

inline hipStream_t S_(void *s) { return reinterpret_cast<hipStream_t>(s); }

constexpr size_t LDS_LIMIT = 160u * 1024u;   // a CU's LDS: the most a workgroup can be given, and only after the opt-in (allow_lds)

inline bool is_f32_planes(int fmt) { return fmt == TRON_OBS_PLANES3_F32 || fmt == TRON_OBS_PLANES4_F32; }

// The TRON_* overrides of the environment, all of them: read once per process, at the first call that looks at one.
//   name                  meaning                                                                         used by
//   TRON_TILE_ENVS        envs per workgroup tile of the per-step kernels (1..64, while the tile fits)    scripts/microbench.py, scripts/stamps.py
//   TRON_ROLL_E           envs per workgroup of the persistent launches                                   scripts/roll_sweep.py
//   TRON_ROLL_WAVES       game waves per workgroup of roll_resident, instead of roll_waves()              A/B runs by hand (the sweep above roll_waves)
//   TRON_ROLL_GRID        workgroups of a persistent launch; below the tile count: k_obs_roll_walk        scripts/roll_sweep.py, tests/test_gpu_rollout_steady.py
//   TRON_ROLL_CHUNK       steps per persistent launch, of BOTH kernel families (64: as they once were)    tests/test_gpu_rollout_long_launch.py, scripts/roll_sweep.py, scripts/roll_fixed_cost.sh
//   TRON_ROLL_PER_STEP    set: every rollout is one launch per step                                       bench.py (A/B switch)
//   TRON_ROLL_FULL_ENTRY  set: every roll_resident launch reads whole planes, as if no mask were valid    A/B runs by hand (the masked entry)
//   TRON_ROLL_NO_HANDOFF  set: every roll_resident launch draws its own first block                       tests/test_gpu_rollout_handoff.py, scripts/roll_stamps.py
//   TRON_ROLL_REPORT      set: k_obs_roll's launch shape (once) and each change of entry, on stderr       by hand (the launch shape)
struct Overrides {
    int tile_envs, roll_e, roll_waves, roll_grid, roll_chunk;      // 0 (or an unusable value): not set
    bool per_step, full_entry, no_handoff, report;
};
const Overrides &overrides()
{
    static const Overrides o = [] {
        auto num = [](const char *name) { const char *v = getenv(name); return v ? atoi(v) : 0; };
        auto set = [](const char *name) { return getenv(name) != nullptr; };
        return Overrides{num("TRON_TILE_ENVS"), num("TRON_ROLL_E"), num("TRON_ROLL_WAVES"), num("TRON_ROLL_GRID"), num("TRON_ROLL_CHUNK"),
                         set("TRON_ROLL_PER_STEP"), set("TRON_ROLL_FULL_ENTRY"), set("TRON_ROLL_NO_HANDOFF"), set("TRON_ROLL_REPORT")};
    }();
    return o;
}

// Does a kernel write the attached planes or the state words (st4 / rs4) outside the hand-over protocol of the roll_resident
// family?  Behind one that does, k_obs_roll's next launch must read whole planes again and draw its own first block (the
// state words' tick and episode may have moved): launch() clears the handle's entry_masks and handed for it.  Every kernel
// of this file has a row; one without does not compile.
template <auto Kernel> struct writes_state;
#define TRON_KERNEL(WRITES, ...) template <> struct writes_state<__VA_ARGS__> : std::bool_constant<WRITES> {}
// k_tile: its step (DO_STEP) moves st4 / rs4 and the handle's own boards; encode-only reads them and writes the caller's
// observations.  k_tile_roll: k_tile's step, k_steps of them.
#define TRON_TILE(F, A) TRON_KERNEL(true, k_tile<F, true, A>); TRON_KERNEL(false, k_tile<F, false, A>); TRON_KERNEL(true, k_tile_roll<F, A>)
TRON_TILE(TRON_OBS_NONE, true); TRON_TILE(TRON_OBS_CODES_I8, true); TRON_TILE(TRON_OBS_PLANES3_F32, true); TRON_TILE(TRON_OBS_PLANES4_F32, true);
TRON_TILE(TRON_OBS_NONE, false); TRON_TILE(TRON_OBS_CODES_I8, false); TRON_TILE(TRON_OBS_PLANES3_F32, false); TRON_TILE(TRON_OBS_PLANES4_F32, false);
#undef TRON_TILE
TRON_KERNEL(true, k_obs<true>);           // a step on the attached planes: planes, st4, rs4
TRON_KERNEL(true, k_obs_slide);           // the sliding modes' step on the attached planes
TRON_KERNEL(true, k_inc<0>);              // the incremental step: the cells a move touches, the boards that restart, st4, rs4
TRON_KERNEL(true, k_obs_roll_walk);       // obs_tile steps that leave no entry mask and hand nothing over
TRON_KERNEL(true, k_obs_roll_slide);      // the same, sliding
TRON_KERNEL(true, k_reset);               // the masked envs' boards, st4 and rs4
TRON_KERNEL(true, k_obs_reset);           // the masked envs' planes, re-derived from their boards
TRON_KERNEL(true, k_obs_attach_marks);    // moves the slide tiles from the planes to the log
TRON_KERNEL(true, k_set_wd);              // rs4 alone, which no entry mask describes: cleared all the same, the call is rare
TRON_KERNEL(false, k_obs_roll);           // the roll_resident family keeps the protocol itself: rollout_wave clears the two
TRON_KERNEL(false, k_obs_roll_tape);      //   flags in front of each of its launches and sets them behind one that was
TRON_KERNEL(false, k_obs_roll_tape_rec);  //   enqueued
TRON_KERNEL(false, k_fresh);              // the fresh-board template, once in tron_create
TRON_KERNEL(false, k_fill_f64);           // the slide rates (P.slide): no plane, no state word
TRON_KERNEL(false, k_obs_planes);         // reads the planes, writes the caller's float planes
TRON_KERNEL(false, k_copy16);             // reads boards or planes, writes the caller's copy
TRON_KERNEL(false, k_obs_to_grid);        // reads the planes, writes the caller's boards
TRON_KERNEL(false, k_obs_grid_marks);     //   and the slide log's tiles into them
TRON_KERNEL(false, k_get_state);          // reads st4 / rs4 / slide
TRON_KERNEL(false, k_encode_codes);       // no handle: the caller's tiles to the caller's codes
TRON_KERNEL(false, k_pop_up);             // no handle: the caller's codes to the caller's planes
#undef TRON_KERNEL

// Every kernel launch of this file.  The LDS opt-in of a kernel that takes dynamic LDS, on first use; the invalidation its
// row of the table asks for; an empty grid (a part without tiles) launches nothing.  h may be null where smem is 0 and the
// kernel writes no state (the entry points without a handle).
template <auto Kernel, class... Args>
int launch(tron_env *h, dim3 grid, dim3 block, size_t smem, hipStream_t st, Args... args)
{
    if (smem) allow_lds<Kernel>(h->device, (int)LDS_LIMIT);
    if constexpr (writes_state<Kernel>::value) h->entry_masks = h->handed = false;
    if (grid.x > 0) hipLaunchKernelGGL(Kernel, grid, block, smem, st, args...);
    return hipGetLastError() == hipSuccess ? TRON_OK : TRON_ERR_LAUNCH;
}

// tiles [tile0, tile0 + blocks) of the handle's current part (all tiles unless a *_part entry point set one)
inline void part_tiles(const tron_env *h, int &tile0, int &blocks)
{
    const int ntiles = (h->P.N + h->E - 1) / h->E;
    const int np = h->nparts > 0 ? h->nparts : 1;
    tile0 = (int)((long long)ntiles * h->part0 / np);
    blocks = (int)((long long)ntiles * (h->part0 + 1) / np) - tile0;
}

// Dynamic LDS of the kernels that run obs_tile (k_obs, k_obs_slide, k_obs_roll_walk, k_obs_roll_slide) on tiles of E envs
size_t obs_tile_smem(const tron_env *h, int E)
{
    return ((size_t)E + 1u) * h->cpe * 16u + 4u * (size_t)E * 16u;
}

// LDS of k_obs_roll (roll_resident): the packed boards, the template, and per game wave the epilogue's store list and the
// helper's rings (on an even dword: one of padding)
size_t roll_smem(const tron_env *h, int E, int waves)
{
    return ((size_t)E * (2u * h->cpe + 1u) + 2u * h->cpe + (size_t)waves * (32u * h->cpe) + 1u + (size_t)waves * ROLL_RING_DWORDS) * 4u;
}

// f(format, aligned): the observation format and the handle's alignment as compile-time constants
template <class F>
int with_fmt(const tron_env *h, int fmt, F f)
{
#define TRON_CASE(FMT)                                                                                               \
    case FMT:                                                                                                        \
        return h->aligned ? f(std::integral_constant<int, FMT>{}, std::true_type{}) : f(std::integral_constant<int, FMT>{}, std::false_type{});
    switch (fmt) {
        TRON_CASE(TRON_OBS_NONE)
        TRON_CASE(TRON_OBS_CODES_I8)
        TRON_CASE(TRON_OBS_PLANES3_F32)
        TRON_CASE(TRON_OBS_PLANES4_F32)
    default:
        return TRON_ERR_BAD_ARG;
    }
#undef TRON_CASE
}

// k_tile over the handle's current part
template <bool DO_STEP>
int launch_fmt(tron_env *h, int fmt, const int8_t *a, const float *u, uint32_t flags, void *obs, StepOut out, hipStream_t st)
{
    int tile0, blocks;
    part_tiles(h, tile0, blocks);
    return with_fmt(h, fmt, [&](auto F, auto A) {
        return launch<k_tile<F(), DO_STEP, A()>>(h, dim3(blocks), dim3(BLOCK), h->smem, st, h->P, h->E, h->cpe, h->cpe_magic, a, u, flags,
                                                 obs, out, tile0);
    });
}

int launch_roll_fmt(tron_env *h, int fmt, int k_steps, uint32_t flags, void *obs, StepOut out, hipStream_t st)
{
    const int ntiles = (h->P.N + h->E - 1) / h->E;
    return with_fmt(h, fmt, [&](auto F, auto A) {
        return launch<k_tile_roll<F(), A()>>(h, dim3(ntiles), dim3(BLOCK), h->smem, st, h->P, h->E, h->cpe, h->cpe_magic, flags, obs, out,
                                             k_steps, ntiles);
    });
}

// one step on the attached planes, over the handle's current part
int launch_obs(tron_env *h, const int8_t *actions, uint32_t flags, StepOut out, hipStream_t st, const float *uniforms = nullptr)
{
    int tile0, blocks;
    part_tiles(h, tile0, blocks);
    const size_t smem = obs_tile_smem(h, h->E);
    if (h->P.mode != TRON_MODE_NONE)                                    // the sliding modes' kernel
        return launch<k_obs_slide>(h, dim3(blocks), dim3(BLOCK), smem, st, h->P, h->E, h->cpe, h->cpe_magic, actions, uniforms, flags,
                                   out, tile0);
    return launch<k_obs<true>>(h, dim3(blocks), dim3(BLOCK), smem, st, h->P, h->E, h->cpe, h->cpe_magic, actions, flags, out, tile0);
}

// one launch of a kernel of the roll_resident family (k_obs_roll takes no tape)
template <auto Kernel>
int launch_roll_resident(tron_env *h, int grid, int waves, size_t smem, hipStream_t st, int E, int epw, uint32_t flags, StepOut out,
                         int steps, const int8_t *tape)
{
    if constexpr (std::is_same_v<decltype(Kernel), decltype(&k_obs_roll)>)
        return launch<Kernel>(h, dim3(grid), dim3(2 * waves * WAVE), smem, st, h->P, E, epw, h->cpe, flags, out, steps, h->emask, h->hand);
    else
        return launch<Kernel>(h, dim3(grid), dim3(2 * waves * WAVE), smem, st, h->P, E, epw, h->cpe, flags, out, steps, tape, h->emask,
                              h->hand);
}

inline int obs_planes(tron_env *h, int fmt, void *obs, hipStream_t st)
{
    const int ch = (fmt == TRON_OBS_PLANES3_F32) ? 3 : 4;
    return launch<k_obs_planes>(h, dim3(4096), dim3(256), 0, st, h->P, ch, reinterpret_cast<float *>(obs));
}

inline bool bad_handle(tron_handle h)
{
    if (!h) return true;
    int dev = -1;
    return hipGetDevice(&dev) != hipSuccess || dev != h->device;
}

}  // namespace

extern "C" {

int tron_abi_version(void) { return TRON_ABI_VERSION; }

const char *tron_strerror(int status)
{
    switch (status) {
    case TRON_OK: return "ok";
    case TRON_ERR_BAD_ARG: return "bad argument";
    case TRON_ERR_NO_DEVICE: return "no HIP device, or the handle's device is not current";
    case TRON_ERR_ALLOC: return "device allocation failed";
    case TRON_ERR_LAUNCH: return "kernel launch failed";
    case TRON_ERR_UNSUPPORTED: return "not supported by this build";
    default: return "unknown status";
    }
}

int tron_synchronize(void *stream)
{
    const hipError_t e = hipStreamSynchronize(S_(stream));
    if (e == hipSuccess) return TRON_OK;
    (void)hipGetLastError();
    return TRON_ERR_LAUNCH;
}

int tron_create(int32_t n_envs, int32_t W, int32_t mode, int32_t fair, uint32_t seed, uint32_t rng_stream,
                tron_handle *out)
{
    if (!out) return TRON_ERR_BAD_ARG;
    *out = nullptr;
    if (n_envs < 1 || W < 2 || W > 96 || mode < TRON_MODE_NONE || mode > TRON_MODE_TEMPER) return TRON_ERR_BAD_ARG;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return TRON_ERR_NO_DEVICE; }

    {   // the slide-threshold table of "temper" mode (g_rate_thr): once per process and device
        static uint64_t filled = 0;
        if (!(filled & (1ull << (dev & 63)))) {
            static float tab[RATE_DEG * RATE_W];
            for (int d = 0; d < RATE_DEG; ++d)
                for (int w = 0; w < RATE_W; ++w) {
                    const double a = (double)((d - 30) - 30) * 0.6;      // game.py:100-102, operation by operation
                    const double b = -a / 100.0;
                    const double c = (double)(70 - (w + 40)) / 100.0;
                    const double rate = b - c;
                    float t = (float)rate;
                    if ((double)t > rate) t = nextafterf(t, -INFINITY);
                    tab[d * RATE_W + w] = t;
                }
            if (hipMemcpyToSymbol(HIP_SYMBOL(g_rate_thr), tab, sizeof(tab)) != hipSuccess) { (void)hipGetLastError(); return TRON_ERR_ALLOC; }
            filled |= 1ull << (dev & 63);
        }
    }
    tron_env *h = new (std::nothrow) tron_env();
    if (!h) return TRON_ERR_ALLOC;
    Params &P = h->P;
    P.N = n_envs; P.W = W; P.S = W + 2; P.G = P.S * P.S; P.mode = mode; P.fair = fair ? 1 : 0;
    P.seed = seed; P.stream = rng_stream;
    P.r_step = -1.0f; P.r_win = 100.0f; P.r_lose = -100.0f; P.r_draw = 0.0f; P.r_index = 0;   // DDQN.py:289-305
    h->device = dev;
    h->side = nullptr; h->fork = nullptr; h->join = nullptr; h->part0 = 0; h->nparts = 1;
    h->entry_masks = h->handed = false;
    h->aligned = (P.G % 4) == 0;
    h->cpe = ((uint32_t)P.G + 15u) / 16u;
    h->cpe_magic = (uint32_t)((0x100000000ull + h->cpe - 1) / h->cpe);   // exact i / cpe for i < 2^32 / cpe

    // tile size: keep the LDS tile near 24 KB so ~6 workgroups share a CU
    int E = (int)((24u * 1024u) / (h->cpe * 16u));
    E = E >= 64 ? 64 : E >= 32 ? 32 : E >= 16 ? 16 : E >= 8 ? 8 : 4;
    const int v = overrides().tile_envs;
    if (v >= 1 && v <= 64 && ((size_t)v + 1u) * h->cpe * 16u + 8192u <= LDS_LIMIT) E = v;
    h->E = E;
    h->smem = ((size_t)E + 1u) * h->cpe * 16u + 3u * (size_t)E * 16u + (size_t)E * 4u + 4u * (((size_t)E * h->cpe + 31u) / 32u + 1u) + 16u;

    // one blob: grid (padded for 16-byte over-read) + state words + fresh template
    const size_t N = (size_t)n_envs;
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    // (sliding modes: the slide-mark log of the observation-is-state layout sits right behind the slide rates: slide_log())
    const size_t log_bytes = P.mode != TRON_MODE_NONE ? N * (size_t)slide_log_len(P.W) * sizeof(uint16_t) : 0;
    const size_t o_grid = 0, o_st4 = align(o_grid + N * P.G + 64), o_rs4 = align(o_st4 + 16 * N),
                 o_slide = align(o_rs4 + 16 * N), o_log = align(o_slide + 8 * N), o_fresh = align(o_log + log_bytes),
                 o_emask = align(o_fresh + (size_t)P.G + 16), o_hand = align(o_emask + 8 * N),
                 total = align(o_hand + 4 * (size_t)ROLL_HAND_DWORDS * N);
    char *blob = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&blob), total) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return TRON_ERR_ALLOC;
    }
    h->blob = blob;
    P.grid = reinterpret_cast<int8_t *>(blob + o_grid);
    P.st4 = reinterpret_cast<uint4 *>(blob + o_st4);
    P.rs4 = reinterpret_cast<uint4 *>(blob + o_rs4);
    P.slide = reinterpret_cast<double *>(blob + o_slide);
    P.obs_state = nullptr;
    P.fresh = reinterpret_cast<const int8_t *>(blob + o_fresh);
    h->emask = reinterpret_cast<unsigned long long *>(blob + o_emask);
    h->hand = reinterpret_cast<uint32_t *>(blob + o_hand);
    if (hipMemsetAsync(blob, 0, total, nullptr) != hipSuccess) { (void)hipGetLastError(); }
    if (launch<k_fresh>(h, dim3((P.G + 255) / 256), dim3(256), 0, nullptr, const_cast<int8_t *>(P.fresh), P.S) != TRON_OK ||
        launch<k_fill_f64>(h, dim3((n_envs + 255) / 256), dim3(256), 0, nullptr, P.slide, 0.15, (const double *)nullptr,
                           n_envs) != TRON_OK ||                                             // config.py:31 slide
        hipStreamSynchronize(nullptr) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(blob);
        delete h;
        return TRON_ERR_LAUNCH;
    }
    *out = h;
    return TRON_OK;
}

int tron_destroy(tron_handle h)
{
    if (!h) return TRON_ERR_BAD_ARG;
    if (h->side) { (void)hipStreamSynchronize(h->side); (void)hipStreamDestroy(h->side); }
    if (h->fork) (void)hipEventDestroy(h->fork);
    if (h->join) (void)hipEventDestroy(h->join);
    (void)hipFree(h->blob);
    delete h;
    return TRON_OK;
}

int tron_info(tron_handle h, int32_t *n_envs, int32_t *W, int32_t *G, int32_t *mode)
{
    if (!h) return TRON_ERR_BAD_ARG;
    if (n_envs) *n_envs = h->P.N;
    if (W) *W = h->P.W;
    if (G) *G = h->P.G;
    if (mode) *mode = h->P.mode;
    return TRON_OK;
}

int tron_set_reward(tron_handle h, float step, float win, float lose, float draw, int32_t step_is_index)
{
    if (!h) return TRON_ERR_BAD_ARG;
    h->P.r_step = step; h->P.r_win = win; h->P.r_lose = lose; h->P.r_draw = draw; h->P.r_index = step_is_index ? 1 : 0;
    return TRON_OK;
}

int tron_set_slide(tron_handle h, double slide, const double *slide_dev, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    return launch<k_fill_f64>(h, dim3((h->P.N + 255) / 256), dim3(256), 0, S_(stream), h->P.slide, slide, slide_dev, h->P.N);
}

int tron_set_weight_degree(tron_handle h, const int16_t *weight, const int16_t *degree, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    return launch<k_set_wd>(h, dim3((h->P.N + 255) / 256), dim3(256), 0, S_(stream), h->P, weight, degree);
}

int tron_reset(tron_handle h, const int8_t *env_mask, const int8_t *start_pos, const int16_t *weight,
               const int16_t *degree, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    const int per = BLOCK / 64;
    int rc = launch<k_reset>(h, dim3((h->P.N + per - 1) / per), dim3(BLOCK), 0, S_(stream), h->P, env_mask, start_pos, weight, degree);
    if (rc == TRON_OK && h->P.obs_state)     // observation-is-state: the masked envs' planes are re-derived from their fresh boards
        rc = launch<k_obs_reset>(h, dim3((h->P.N + per - 1) / per), dim3(BLOCK), 0, S_(stream), h->P, env_mask);
    return rc;
}

int tron_attach_obs_state(tron_handle h, int8_t *obs_codes, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if (!obs_codes || (reinterpret_cast<uintptr_t>(obs_codes) & 15u)) return TRON_ERR_BAD_ARG;
    if (!h->aligned || h->P.G >= 0x3FFF) return TRON_ERR_UNSUPPORTED;                 // (cell + 1 travels in 14 bits: restart word, slide marks)
    if (h->P.obs_state) return TRON_ERR_BAD_ARG;                                      // already attached
    h->entry_masks = h->handed = false;   // the planes are another buffer from here on, whatever the launches below do
    h->P.obs_state = obs_codes;
    const int per = BLOCK / 64;     // derive the planes from the boards as they are now
    int rc = launch<k_obs_reset>(h, dim3((h->P.N + per - 1) / per), dim3(BLOCK), 0, S_(stream), h->P, (const int8_t *)nullptr);
    if (rc == TRON_OK && h->P.mode != TRON_MODE_NONE)  // slide tiles are not codable (Map.color shows them as bodies): they go to the log (lane_move_codes_slide)
        rc = launch<k_obs_attach_marks>(h, dim3((h->P.N + 255) / 256), dim3(256), 0, S_(stream), h->P);
    return rc;
}

int tron_step_encode(tron_handle h, const int8_t *actions, const float *uniforms, uint32_t flags, int32_t obs_fmt,
                     void *obs, int8_t *out_done, int8_t *out_winner, float *out_reward, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if ((obs_fmt != TRON_OBS_NONE) != (obs != nullptr)) return TRON_ERR_BAD_ARG;
    if (flags & ~(TRON_STEP_AUTORESET | TRON_STEP_INCREMENTAL | TRON_STEP_NONREVERSING)) return TRON_ERR_BAD_ARG;
    if ((flags & TRON_STEP_INCREMENTAL) && (!h->P.obs_state || h->P.mode != TRON_MODE_NONE)) return TRON_ERR_UNSUPPORTED;
    StepOut out{out_done, out_winner, out_reward, nullptr};
    if (h->P.obs_state) {
        if (obs_fmt == TRON_OBS_CODES_I8 && obs != h->P.obs_state) return TRON_ERR_BAD_ARG;   // the attached buffer is the output
        if (obs_fmt < TRON_OBS_NONE || obs_fmt > TRON_OBS_PLANES4_F32) return TRON_ERR_BAD_ARG;
        const int rc = (flags & TRON_STEP_INCREMENTAL)
                           ? launch<k_inc<0>>(h, dim3((h->P.N + WAVE - 1) / WAVE), dim3(BLOCK), 0, S_(stream), h->P, h->cpe, actions, flags, out)
                           : launch_obs(h, actions, flags, out, S_(stream), uniforms);
        if (rc != TRON_OK || !is_f32_planes(obs_fmt)) return rc;
        return obs_planes(h, obs_fmt, obs, S_(stream));
    }
    return launch_fmt<true>(h, obs_fmt, actions, uniforms, flags, obs, out, S_(stream));
}

int tron_step(tron_handle h, const int8_t *actions, const float *uniforms, uint32_t flags, int8_t *out_done,
              int8_t *out_winner, float *out_reward, void *stream)
{
    return tron_step_encode(h, actions, uniforms, flags, TRON_OBS_NONE, nullptr, out_done, out_winner, out_reward,
                            stream);
}

int tron_part_range(tron_handle h, int32_t part, int32_t nparts, int32_t *first_env, int32_t *n_envs)
{
    if (!h || nparts < 1 || part < 0 || part >= nparts) return TRON_ERR_BAD_ARG;
    const int ntiles = (h->P.N + h->E - 1) / h->E;
    const long long t0 = (long long)ntiles * part / nparts, t1 = (long long)ntiles * (part + 1) / nparts;
    const long long e0 = t0 * h->E, e1 = t1 * h->E < h->P.N ? t1 * h->E : h->P.N;
    if (first_env) *first_env = (int32_t)e0;
    if (n_envs) *n_envs = (int32_t)(e1 - e0);
    return TRON_OK;
}

int tron_step_encode_part(tron_handle h, int32_t part, int32_t nparts, const int8_t *actions, const float *uniforms,
                          uint32_t flags, int32_t obs_fmt, void *obs, int8_t *out_done, int8_t *out_winner,
                          float *out_reward, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if (nparts < 1 || part < 0 || part >= nparts) return TRON_ERR_BAD_ARG;
    if (flags & TRON_STEP_INCREMENTAL) return TRON_ERR_UNSUPPORTED;
    if (h->P.obs_state && is_f32_planes(obs_fmt)) return TRON_ERR_UNSUPPORTED;
    h->part0 = part;
    h->nparts = nparts;
    const int rc = tron_step_encode(h, actions, uniforms, flags, obs_fmt, obs, out_done, out_winner, out_reward, stream);
    h->part0 = 0;
    h->nparts = 1;
    return rc;
}

int tron_encode(tron_handle h, int32_t obs_fmt, void *obs, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if (obs_fmt == TRON_OBS_NONE || !obs) return TRON_ERR_BAD_ARG;
    StepOut out{nullptr, nullptr, nullptr, nullptr};
    if (h->P.obs_state) {
        if (obs_fmt == TRON_OBS_CODES_I8) {
            if (obs == h->P.obs_state) return TRON_OK;            // the attached planes are always current
            const size_t nbytes = (size_t)h->P.N * 2u * h->P.G;
            if (reinterpret_cast<uintptr_t>(obs) & 15u) return TRON_ERR_BAD_ARG;
            return launch<k_copy16>(h, dim3(2048), dim3(256), 0, S_(stream), reinterpret_cast<const uint4 *>(h->P.obs_state),
                                    reinterpret_cast<uint4 *>(obs), nbytes / 16, h->P.obs_state, reinterpret_cast<int8_t *>(obs), nbytes);
        }
        if (!is_f32_planes(obs_fmt)) return TRON_ERR_BAD_ARG;
        return obs_planes(h, obs_fmt, obs, S_(stream));
    }
    return launch_fmt<false>(h, obs_fmt, nullptr, nullptr, 0u, obs, out, S_(stream));
}

int tron_get_grid(tron_handle h, int8_t *grid_out, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if (!grid_out) return TRON_ERR_BAD_ARG;
    if (h->P.obs_state) {
        int rc = launch<k_obs_to_grid>(h, dim3(2048), dim3(256), 0, S_(stream), h->P, grid_out);
        if (rc == TRON_OK && h->P.mode != TRON_MODE_NONE)
            rc = launch<k_obs_grid_marks>(h, dim3((h->P.N + 255) / 256), dim3(256), 0, S_(stream), h->P, grid_out);
        return rc;
    }
    const size_t nbytes = (size_t)h->P.N * h->P.G;
    const bool aligned = (reinterpret_cast<uintptr_t>(grid_out) & 15u) == 0;
    const size_t n16 = aligned ? nbytes / 16 : 0;
    const int blocks = (int)((n16 / 256 < 2048 ? n16 / 256 : 2048) + 1);
    return launch<k_copy16>(h, dim3(blocks), dim3(256), 0, S_(stream), reinterpret_cast<const uint4 *>(h->P.grid),
                            reinterpret_cast<uint4 *>(grid_out), n16, h->P.grid, grid_out, nbytes);
}

int tron_get_state(tron_handle h, int8_t *pos, int8_t *alive, int8_t *dir, int8_t *done, int8_t *winner,
                   int16_t *weight, int16_t *degree, double *slide, uint32_t *counters, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    return launch<k_get_state>(h, dim3((h->P.N + 255) / 256), dim3(256), 0, S_(stream), h->P, pos, alive, dir, done, winner, weight,
                               degree, slide, counters);
}

namespace {

// k_steps steps of the observation-is-state kernel as persistent launches of at most TRON_ROLLOUT_CHUNK steps (k_obs_roll and
// its tape forms: ROLL_LAUNCH_CAP, above rollout_wave), one tile per
// workgroup: with more workgroups than the chip holds at once the late ones start as the early ones finish their steps.
// Tile size for the kernels that run obs_tile every step (the sliding modes; k_obs_roll_walk has the same code and occupancy
// and is what is asked here).  The chip holds `slots` workgroups at once (occupancy x CUs), so the launch runs in
// ceil(ntiles / slots) rounds and the last one should be full.  Picks the E in [3/4 E0, E0] with the fullest last round
// (E0 = the per-step kernels' tile); small batches that fit in one round keep E0.
int roll_tile_envs(const tron_env *h)
{
    const int E0 = h->E;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) { (void)hipGetLastError(); return E0; }
    allow_lds<k_obs_roll_walk>(h->device, (int)LDS_LIMIT);                   // (the query below is made in front of its first launch)
    int best = E0;
    double best_fill = -1.0;
    for (int E = E0; E >= (3 * E0 + 3) / 4 && E >= 1; --E) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_obs_roll_walk, BLOCK, obs_tile_smem(h, E)) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            continue;
        }
        const double slots = (double)per_cu * prop.multiProcessorCount;
        const double rounds = ((h->P.N + E - 1) / E) / slots;
        if (rounds <= 1.0) return E == E0 ? E0 : best;                  // everything resident at once: nothing to balance
        const double fill = rounds / (double)(long long)(rounds + 0.999999);
        if (fill > best_fill + 0.02) { best_fill = fill; best = E; }    // prefer the larger tile unless clearly fuller
    }
    return best;
}

// Mode None on boards of at most 64 chunks (sides up to 30): k_obs_roll, one lane per env.  Envs per wave x waves per
// workgroup, swept at 65 536 x 24x24 (us per step at 64 steps per launch; parent 13.1; the 20-step form is in
// profiles/r07_rollout_ab.txt):  64 x 1: 6.90   64 x 2: 8.41   64 x 4: 6.66   32 x 1: 7.85   32 x 2: 7.92   32 x 4: 7.84
// 16 x 1: 11.04   16 x 2: 11.03   16 x 4: 10.99
// Full waves win: the step is bound by the instructions a SIMD issues, and a wave of 16 or 32 envs issues as many as one of
// 64, so two or four narrow waves per SIMD cost what they were meant to hide.  Four waves of 64 per workgroup take 110 KB of
// LDS at 24x24 (89 KB of boards, 22 KB of store lists: 111 448 B): one workgroup per CU and one wave per SIMD wherever the dispatcher puts them, where 1 024 one-wave or 512
// two-wave workgroups land unevenly (64 x 2: some CUs hold three).  Repeated runs of 64 x 1 against 64 x 4 are in
// profiles/r07_rollout_ab.txt.  A batch with no more 64-env waves than the chip has CUs gets one wave per workgroup, so that
// it spreads over the CUs: a rule of thumb, not measured (the sweep is at 65 536 envs only).  Chosen once per handle.
constexpr int ROLL_EPW = 64;
int roll_waves(tron_env *h)
{
    if (!h->roll_waves) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) { (void)hipGetLastError(); cus = 0; }
        h->roll_waves = (h->P.N + ROLL_EPW - 1) / ROLL_EPW > cus ? BLOCK / WAVE : 1;
    }
    return h->roll_waves;
}

// Steps per launch of the roll_resident family (k_obs_roll, k_obs_roll_tape, k_obs_roll_tape_rec): the whole call, up to this
// many.  A launch pays its prologue, its epilogue and the ramp and tail of the grid once, about 20 us at 65 536 x 24x24
// where a step is 0.8 us: a quarter of a 64-step launch (TRON_ROLLOUT_CHUNK, chosen when a step was 20 us and still the
// other kernels' length), and between two launches stands a device-wide barrier between workgroups that exchange nothing,
// with an epilogue that stores what the next prologue loads straight back.  At 1 024 steps the fixed share is 2 % — nothing
// left worth a longer launch — and a launch stays near 1 ms, so that a call of 100 000 steps does not hold the chip in one
// dispatch: it splits into launches of the cap, the remainder last, as it always split at 64.  Nothing in the kernel counts
// on a length: the byte tallies are flushed every 128 steps, the start ring is keyed by the absolute episode and
// topped up by count, restart counts, ticks and rows are 32-bit and wider.  TRON_ROLL_CHUNK overrides it (A/B runs:
// TRON_ROLL_CHUNK=64 is the launches as they were; scripts/roll_sweep.py, scripts/roll_fixed_cost.sh).
constexpr int ROLL_LAUNCH_CAP = 1024;
static_assert(ROLL_LAUNCH_CAP % 128 == 0, "whole tally periods and whole blocks: the launches of a long call are all alike");

// out with its record tapes `envs` entries on (a step is N of them): the rows of a later step; a null tape stays null
inline StepOut rows_from(StepOut out, size_t envs)
{
    return StepOut{out.done ? out.done + envs : nullptr, out.winner ? out.winner + envs : nullptr,
                   out.reward ? out.reward + 2u * envs : nullptr, out.totals};
}

// TRON_ROLL_REPORT: the launch shape and its occupancy on stderr, once per process
void report_roll_shape(const tron_env *h, int E, int waves, int epw, size_t smem, int grid)
{
    static bool reported = false;
    if (reported) return;
    reported = true;
    allow_lds<k_obs_roll>(h->device, (int)LDS_LIMIT);
    int per_cu = 0;
    hipDeviceProp_t prop;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_obs_roll, 2 * waves * WAVE, smem) == hipSuccess &&
        hipGetDeviceProperties(&prop, h->device) == hipSuccess)
        fprintf(stderr, "k_obs_roll: %d envs per workgroup, %d game waves of %d envs and as many helper waves, %zu B of LDS, grid %d; %d workgroups per CU x %d CUs = %d resident\n",
                E, waves, epw, smem, grid, per_cu, prop.multiProcessorCount, per_cu * prop.multiProcessorCount);
    (void)hipGetLastError();
}

// TRON_ROLL_REPORT: the entry a launch takes, whenever it is not the last one reported
void report_roll_entry(uint32_t flags, int steps, bool tape)
{
    static int reported = -1;
    const int entry = (flags & ROLL_ENTRY_MASKED ? 1 : 0) | (flags & ROLL_ENTRY_HANDED ? 2 : 0);
    if (entry != reported)
        fprintf(stderr, "k_obs_roll: a launch of %d steps enters by %s, its first block's starts%s %s\n", steps,
                entry & 1 ? "the entry masks" : "whole planes", tape ? "" : " and actions", entry & 2 ? "handed over" : "drawn");
    reported = entry;
}

// tape: null for k_obs_roll's own draws; else the caller's int8[k_steps][N][2], and every launch gets it advanced to its
// own first step (k_obs_roll_tape: same grid, same workgroup, same LDS).  A tape call that asks for records (any of
// out.done / out.winner / out.reward) runs k_obs_roll_tape_rec, and its launches get the record tapes advanced by the same rows.
int rollout_wave(tron_env *h, int32_t k_steps, uint32_t flags_in, StepOut out, hipStream_t st, int E, int waves, int chunk,
                 const int8_t *tape = nullptr)
{
    if (waves < 1) waves = 1;
    if (E > waves * WAVE) waves = (E + WAVE - 1) / WAVE;            // at most 64 envs per wave
    if (waves > BLOCK / WAVE) return TRON_ERR_BAD_ARG;
    const int epw = (E + waves - 1) / waves;
    const int grid = (h->P.N + E - 1) / E;
    const size_t smem = roll_smem(h, E, waves);
    if (smem > LDS_LIMIT) return TRON_ERR_BAD_ARG;
    const bool rec = tape && (out.done || out.winner || out.reward);
    const auto launch_it = rec ? &launch_roll_resident<k_obs_roll_tape_rec> : tape ? &launch_roll_resident<k_obs_roll_tape>
                                                                                   : &launch_roll_resident<k_obs_roll>;
    const Overrides &o = overrides();
    if (o.report) report_roll_shape(h, E, waves, epw, smem, grid);
    const bool autoreset = (flags_in & TRON_STEP_AUTORESET) != 0u;
    for (int done = 0; done < k_steps; done += chunk) {
        // The launch covers all envs (grid x E >= N) and writes every env's entry mask; the one behind it on the stream may
        // enter by them.  Nothing is assumed of a launch that failed.
        // It hands its helper's rings over as well (autoreset alone); the one behind it takes them if it would draw the same
        // words: same seed, stream, fair and W.
        const int steps = k_steps - done < chunk ? k_steps - done : chunk;
        const bool take = h->handed && autoreset && !o.no_handoff && h->hand_seed == h->P.seed && h->hand_stream == h->P.stream &&
                          h->hand_fair == h->P.fair && h->hand_W == h->P.W;
        const uint32_t flags = flags_in | (h->entry_masks && !o.full_entry ? ROLL_ENTRY_MASKED : 0u) | (take ? ROLL_ENTRY_HANDED : 0u);
        h->entry_masks = h->handed = false;
        if (o.report) report_roll_entry(flags, steps, tape != nullptr);
        const size_t at = (size_t)done * (size_t)h->P.N;              // the launch's first row, in envs (record tapes: behind a tape alone)
        if (launch_it(h, grid, waves, smem, st, E, epw, flags, rows_from(out, at), steps, tape ? tape + 2u * at : nullptr) != TRON_OK)
            return TRON_ERR_LAUNCH;
        h->entry_masks = true;
        h->handed = autoreset;
        h->hand_seed = h->P.seed; h->hand_stream = h->P.stream; h->hand_fair = h->P.fair; h->hand_W = h->P.W;
    }
    return TRON_OK;
}

// tape != null (tron_rollout_actions): TRON_ERR_UNSUPPORTED wherever the launch would not be k_obs_roll's shape — the
// caller then steps per launch.
int rollout_persistent(tron_env *h, int32_t k_steps, uint32_t flags, StepOut out, hipStream_t st, const int8_t *tape = nullptr)
{
    const Overrides &o = overrides();
    // chunk: steps per launch of the kernels that run obs_tile every step (k_obs_roll_walk, k_obs_roll_slide);
    // wave_chunk: of the roll_resident family (ROLL_LAUNCH_CAP).  TRON_ROLL_CHUNK sets both.
    const int chunk = o.roll_chunk > 0 ? o.roll_chunk : TRON_ROLLOUT_CHUNK, wave_chunk = o.roll_chunk > 0 ? o.roll_chunk : ROLL_LAUNCH_CAP;
    const bool sliding = h->P.mode != TRON_MODE_NONE;
    if (!sliding && h->cpe <= 64u) {
        // (mode None ONLY: k_obs_roll leaves rs4.envp / rs4.nenvp alone until its epilogue, which no sliding step could bear)
        // TRON_ROLL_E stays envs per workgroup, TRON_ROLL_WAVES its waves; a TRON_ROLL_GRID below the workgroup count asks for
        // the walking kernel below
        int waves = o.roll_waves > 0 ? o.roll_waves : roll_waves(h);
        // 30x30 (64 chunks): four waves' boards and lists (165 376 B) are past the 160 KB of a CU, three fit (124 160 B).  TRON_ROLL_WAVES is clamped
        // the same way; a TRON_ROLL_E that needs more waves than fit (256 envs at 30x30) is TRON_ERR_BAD_ARG in rollout_wave.
        while (o.roll_e <= 0 && waves > 1 && roll_smem(h, waves * ROLL_EPW, waves) > LDS_LIMIT) --waves;
        const int E = o.roll_e > 0 ? o.roll_e : waves * ROLL_EPW;
        if (!(o.roll_grid > 0 && o.roll_grid < (h->P.N + E - 1) / E)) return rollout_wave(h, k_steps, flags, out, st, E, waves, wave_chunk, tape);
    }
    if (tape) return TRON_ERR_UNSUPPORTED;
    if (!h->roll_E) h->roll_E = roll_tile_envs(h);
    // obs_tile every step (the sliding modes; mode None on boards of more than 64 chunks or with TRON_ROLL_GRID: k_obs_roll_walk).
    // The sliding modes: the per-step tile for a call that fits ONE launch and for the resident variant, else the tile with the
    // fullest last round — measured at 65 536 x 24x24.  Mode None: the per-step tile.
    const int E = o.roll_e > 0 ? o.roll_e : !sliding ? h->E : ((flags & TRON_ROLLOUT_RESIDENT) || k_steps <= chunk) ? h->E : h->roll_E;
    const int ntiles = (h->P.N + E - 1) / E;
    const int grid = (o.roll_grid > 0 && o.roll_grid < ntiles) ? o.roll_grid : ntiles;
    const size_t smem = obs_tile_smem(h, E);
    if (smem > LDS_LIMIT) return TRON_ERR_BAD_ARG;
    for (int left = k_steps; left > 0; left -= chunk) {
        const int steps = left < chunk ? left : chunk;
        const int rc = sliding ? launch<k_obs_roll_slide>(h, dim3(grid), dim3(BLOCK), smem, st, h->P, E, h->cpe, h->cpe_magic, flags, out, steps, ntiles)
                               : launch<k_obs_roll_walk>(h, dim3(grid), dim3(BLOCK), smem, st, h->P, E, h->cpe, h->cpe_magic, flags, out, steps, ntiles);
        if (rc != TRON_OK) return TRON_ERR_LAUNCH;
    }
    return TRON_OK;
}

// actions: null for the env's own draws; else a tape of [k_steps][N][2] for launches of one step each (TRON_ROLLOUT_PER_STEP),
// with row k of out's record tapes to step k
int rollout_launches(tron_env *h, int32_t k_steps, uint32_t flags, int32_t obs_fmt, void *obs, StepOut out, hipStream_t st,
                     const int8_t *actions = nullptr)
{
    const bool two_streams = (flags & TRON_ROLLOUT_TWO_STREAMS) != 0u;
    if (!(h->P.obs_state && !(flags & (TRON_ROLLOUT_PER_STEP | TRON_ROLLOUT_TWO_STREAMS)))) flags &= ~TRON_ROLLOUT_RESIDENT;   // persistent obs-is-state launches only
    const bool per_step = overrides().per_step || two_streams || (flags & TRON_ROLLOUT_PER_STEP) != 0u;
    flags &= ~(TRON_ROLLOUT_PER_STEP | TRON_ROLLOUT_TWO_STREAMS);
    if (h->P.obs_state && !per_step && k_steps > 1) {
        const int rc = rollout_persistent(h, k_steps, flags, out, st);
        if (rc != TRON_OK) return rc;
        return is_f32_planes(obs_fmt) ? obs_planes(h, obs_fmt, obs, st) : TRON_OK;
    }
    flags &= ~TRON_ROLLOUT_RESIDENT;                               // only k_obs_roll knows it
    if (!h->P.obs_state && !per_step && k_steps > 1) {             // board-owning layout: same idea, k_tile_roll
        for (int left = k_steps; left > 0; left -= TRON_ROLLOUT_CHUNK) {
            const int rc = launch_roll_fmt(h, obs_fmt, left < TRON_ROLLOUT_CHUNK ? left : TRON_ROLLOUT_CHUNK, flags, obs, out, st);
            if (rc != TRON_OK) return rc;
        }
        return TRON_OK;
    }
    // One launch per step; TRON_ROLLOUT_TWO_STREAMS: per step and per half of the envs.  The env batch as two independent
    // halves, each a launch sequence of its own on its own stream: a half's step s+1 only depends on its own step s, so the
    // drain of one half's launch overlaps the ramp-up of the other's.  Fork / join events order both against what came
    // before and comes after on `st`.
    const int parts = two_streams && k_steps > 0 ? 2 : 1;
    if (parts == 2) {
        if (!h->side) {
            if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
                hipEventCreateWithFlags(&h->fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&h->join, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                return TRON_ERR_ALLOC;
            }
        }
        if (hipEventRecord(h->fork, st) != hipSuccess || hipStreamWaitEvent(h->side, h->fork, 0) != hipSuccess) {
            (void)hipGetLastError();
            return TRON_ERR_LAUNCH;
        }
    }
    const size_t n = (size_t)h->P.N;
    int rc = TRON_OK;
    h->nparts = parts;
    for (int k = 0; k < k_steps && rc == TRON_OK; ++k)
        for (int part = 0; part < parts && rc == TRON_OK; ++part) {
            h->part0 = part;
            hipStream_t s2 = part ? h->side : st;
            const int8_t *a = actions ? actions + 2u * (k * n) : nullptr;
            rc = h->P.obs_state ? launch_obs(h, a, flags, rows_from(out, k * n), s2)
                                : launch_fmt<true>(h, obs_fmt, a, nullptr, flags, obs, rows_from(out, k * n), s2);
        }
    h->part0 = 0;
    h->nparts = 1;
    if (parts == 2 && (hipEventRecord(h->join, h->side) != hipSuccess || hipStreamWaitEvent(st, h->join, 0) != hipSuccess)) {
        (void)hipGetLastError();
        return TRON_ERR_LAUNCH;
    }
    if (rc != TRON_OK) return rc;
    if (h->P.obs_state && is_f32_planes(obs_fmt) && k_steps > 0)
        return obs_planes(h, obs_fmt, obs, st);
    return TRON_OK;
}

}  // namespace

int tron_rollout_random(tron_handle h, int32_t k_steps, uint32_t flags, int32_t obs_fmt, void *obs,
                        unsigned long long *totals, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if (k_steps < 0 || (obs_fmt != TRON_OBS_NONE) != (obs != nullptr)) return TRON_ERR_BAD_ARG;
    if (flags & ~(TRON_STEP_NONREVERSING | TRON_ROLLOUT_PER_STEP | TRON_ROLLOUT_TWO_STREAMS | TRON_ROLLOUT_RESIDENT))
        return TRON_ERR_BAD_ARG;   // autoreset is implied
    StepOut out{nullptr, nullptr, nullptr, totals};
    if (h->P.obs_state && obs_fmt == TRON_OBS_CODES_I8 && obs != h->P.obs_state) return TRON_ERR_BAD_ARG;
    return rollout_launches(h, k_steps, flags | TRON_STEP_AUTORESET, obs_fmt, obs, out, S_(stream));
}

int tron_rollout_actions(tron_handle h, int32_t k_steps, const int8_t *actions, uint32_t flags, int32_t obs_fmt, void *obs,
                         unsigned long long *totals, void *stream)
{
    return tron_rollout_actions_records(h, k_steps, actions, flags, obs_fmt, obs, nullptr, nullptr, nullptr, totals, stream);
}

int tron_rollout_actions_records(tron_handle h, int32_t k_steps, const int8_t *actions, uint32_t flags, int32_t obs_fmt, void *obs,
                                 int8_t *out_done, int8_t *out_winner, float *out_reward, unsigned long long *totals, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if (!actions || k_steps < 0 || (obs_fmt != TRON_OBS_NONE) != (obs != nullptr)) return TRON_ERR_BAD_ARG;
    if (flags & ~TRON_ROLLOUT_PER_STEP) return TRON_ERR_BAD_ARG;    // autoreset is implied; a tape has no policy to flag
    if (obs_fmt < TRON_OBS_NONE || obs_fmt > TRON_OBS_PLANES4_F32) return TRON_ERR_BAD_ARG;
    if (h->P.obs_state && obs_fmt == TRON_OBS_CODES_I8 && obs != h->P.obs_state) return TRON_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(out_reward) & 7u) return TRON_ERR_BAD_ARG;   // a row is float2 stores
    // the record tapes (any of them null): k_obs_roll_tape_rec in the persistent launches, row k to step k below
    StepOut out{out_done, out_winner, out_reward, totals};
    hipStream_t st = S_(stream);
    // the persistent launches: mode None on the attached codes (k_obs_roll_tape); a single step is one per-step launch
    if (h->P.obs_state && h->P.mode == TRON_MODE_NONE && !is_f32_planes(obs_fmt) && !(flags & TRON_ROLLOUT_PER_STEP) && k_steps > 1) {
        const int rc = rollout_persistent(h, k_steps, TRON_STEP_AUTORESET, out, st, actions);
        if (rc != TRON_ERR_UNSUPPORTED) return rc;                   // (boards past 64 chunks, a TRON_ROLL_GRID override: below)
    }
    // everywhere else: tron_step_encode's launch with row k, and the totals tron_rollout_random's per-step form keeps
    return rollout_launches(h, k_steps, TRON_STEP_AUTORESET | TRON_ROLLOUT_PER_STEP, obs_fmt, obs, out, st, actions);
}

int tron_minimax_actions(tron_handle h, int32_t player, int32_t depth, int32_t mode, int8_t *out_actions,
                         int32_t *out_values, int8_t *out_expanded, void *stream)
{
    if (bad_handle(h)) return h ? TRON_ERR_NO_DEVICE : TRON_ERR_BAD_ARG;
    if (!out_actions || (player != 1 && player != 2)) return TRON_ERR_BAD_ARG;
    if (mode != TRON_MINIMAX_VORONOI && mode != TRON_MINIMAX_DISTWALL) return TRON_ERR_BAD_ARG;
    if (depth != 2 || h->P.S > 64) return TRON_ERR_UNSUPPORTED;
    MinimaxSrc src{};
    if (h->P.obs_state) {       // the attached planes are the boards: player p's plane is its observation
        src.codes = h->P.obs_state + (size_t)(player - 1) * (size_t)h->P.G;
        src.stride = 2u * (size_t)h->P.G;
    } else {
        src.grid = h->P.grid;
    }
    src.player = player;
    src.st4 = h->P.st4;
    src.seed = h->P.seed;
    src.stream = h->P.stream;
    return launch_minimax(src, h->P.N, h->P.S, mode, out_actions, out_values, out_expanded, S_(stream));
}

int tron_encode_codes(const int8_t *tiles, int64_t n, int32_t cells, int32_t player, int8_t *codes_out, void *stream)
{
    if (!tiles || !codes_out || n < 0 || cells < 1 || (player != 1 && player != 2)) return TRON_ERR_BAD_ARG;
    const size_t nbytes = (size_t)n * (size_t)cells;
    if (nbytes == 0) return TRON_OK;
    if ((reinterpret_cast<uintptr_t>(tiles) | reinterpret_cast<uintptr_t>(codes_out)) & 15u) return TRON_ERR_BAD_ARG;
    size_t blocks = (nbytes / 16 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    return launch<k_encode_codes>(nullptr, dim3((unsigned)blocks), dim3(256), 0, S_(stream), tiles, nbytes, player == 2, codes_out);
}

int tron_pop_up(const int8_t *codes, int64_t n, int32_t cells, float *planes_out, void *stream)
{
    if (!codes || !planes_out || n < 0 || cells < 1) return TRON_ERR_BAD_ARG;
    if (n == 0) return TRON_OK;
    size_t blocks = ((size_t)n * cells + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return launch<k_pop_up>(nullptr, dim3((unsigned)blocks), dim3(256), 0, S_(stream), codes, (size_t)n, cells, planes_out);
}

}  // extern "C"
