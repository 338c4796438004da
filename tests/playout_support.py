"""What the playout tests share (tests/test_playout_model_cpu.py, tests/test_gpu_playout.py): a host model of
tron_playout_codes built on the CPU oracle, and the boards and tapes both files use.  The model decodes player 1's code
images to Tile grids and head positions, steps them with the oracle's orc_step in mode None (through VecOracle, whose
arrays it fills), encodes with state_for_player, and draws safe moves from the oracle's Philox as include/tron_hip.h
states them.  A plain module, imported by name; nothing here needs a GPU."""
import ctypes as C

import numpy as np

import oracle
from rollout_support import start_positions

EMPTY, WALL, P1_BODY, P1_HEAD, P2_BODY, P2_HEAD = 0, -1, 1, 2, 3, 4      # raw tile values (map.py:9-17)
CLASSES = ("p1_wins", "p2_wins", "same_cell", "both_crash", "border_deaths", "unfinished", "boxed_in", "rejected")
DR = np.array([-1, 0, 1, 0])                                           # UP, RIGHT, DOWN, LEFT (player.py:124-132)
DC = np.array([0, 1, 0, -1])

_TILE_OF_CODE = np.full(256, WALL, np.int8)                            # any byte that is no code reads as a wall
for _code, _tile in ((1, EMPTY), (-1, WALL), (-2, P1_BODY), (-3, P2_BODY), (10, P1_HEAD), (-10, P2_HEAD)):
    _TILE_OF_CODE[_code & 0xFF] = _tile


def decode(codes):
    """[n, S, S] player-1 codes -> (tiles int8 [n, S*S], pos int8 [n, 4] board coordinates, playable bool [n]).
    Playable: exactly one +10 and one -10, both strictly inside the border; pos of the others is 0."""
    codes = np.ascontiguousarray(codes, np.int8)
    n, S = codes.shape[0], codes.shape[-1]
    flat = codes.reshape(n, S * S)
    tiles = _TILE_OF_CODE[flat.view(np.uint8)]
    pos = np.zeros((n, 4), np.int8)
    playable = np.ones(n, bool)
    for p, head in enumerate((10, -10)):
        is_head = flat == head
        at = is_head.argmax(1)
        r, c = at // S, at % S
        playable &= (is_head.sum(1) == 1) & (r >= 1) & (c >= 1) & (r <= S - 2) & (c <= S - 2)
        pos[:, 2 * p], pos[:, 2 * p + 1] = r - 1, c - 1
    pos[~playable] = 0
    return tiles, pos, playable


class _Philox:
    """The oracle's Philox-4x32-10, one block per call, without an allocation per call."""

    def __init__(self, seed, stream, call):
        self.ctr = np.zeros(4, np.uint32)
        self.key = np.array([seed & 0xFFFFFFFF, stream & 0xFFFFFFFF], np.uint32)
        self.out = np.zeros(4, np.uint32)
        self.ctr[2], self.ctr[3] = call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF
        self.fn = oracle.lib().orc_philox4x32_10
        self.args = tuple(C.c_void_p(a.ctypes.data) for a in (self.ctr, self.key, self.out))

    def words(self, index, step):
        self.ctr[0], self.ctr[1] = index, step
        self.fn(*self.args)
        return self.out


class Playouts:
    """n boards under mode None's rule, stepped together.  step(row) plays one step of every playout that is still
    live: row int8 [n, 2], a byte 0..127 an action (its low two bits), a negative byte a safe draw."""

    def __init__(self, codes, seed=0x5EED, stream_id=0, call=0, first_index=0):
        self.codes = np.ascontiguousarray(codes, np.int8)
        self.n, self.S = self.codes.shape[0], self.codes.shape[-1]
        self.W = self.S - 2
        tiles, pos, self.playable = decode(self.codes)
        self.v = v = oracle.VecOracle(self.n, self.W, mode=None)
        v.grid[:], v.pos[:], v.done[:] = tiles, pos, ~self.playable
        self.philox = _Philox(seed, stream_id, call)
        self.first_index = first_index                                 # playout i is index first_index + i of its launch
        self.t = 0
        self.boxed_in = np.zeros(self.n, bool)                         # a safe draw found no candidate
        self.zeros = np.zeros((self.n, 2), np.float32)

    def live(self):
        return self.v.done == 0

    def safe_moves(self, need):
        """[n, 2] the safe draw of every (playout, player) in `need`, 0 elsewhere."""
        v, S = self.v, self.S
        out = np.zeros((self.n, 2), np.int8)
        rows = np.nonzero(need.any(1))[0]
        if not len(rows):
            return out
        pos = v.pos[rows].astype(np.int64).reshape(-1, 2, 2)           # [m, player, (r, c)]
        cell = (pos[:, :, 0] + 1) * S + (pos[:, :, 1] + 1)
        target = cell[:, :, None] + (DR * S + DC)[None, None, :]       # [m, 2, 4] in UP, RIGHT, DOWN, LEFT order
        free = v.grid[rows[:, None, None], target] == EMPTY            # the board as it stands: a head is no empty cell
        cnt = free.sum(2)
        u = np.array([self.philox.words(self.first_index + i, self.t)[:2].copy() for i in rows], np.uint64)
        pick = (u * cnt.astype(np.uint64)) >> np.uint64(32)            # mulhi(u, c)
        rank = np.cumsum(free, 2) - 1                                  # a candidate's place in the list
        move = (free & (rank == pick[:, :, None].astype(np.int64))).argmax(2)   # none: argmax of all False = 0 = UP
        out[rows] = np.where(need[rows], move, 0)
        self.boxed_in[rows] |= (need[rows] & (cnt == 0)).any(1)
        return out

    def step(self, row=None):
        live = self.live()
        row = np.full((self.n, 2), -1, np.int8) if row is None else np.asarray(row, np.int8)
        need = live[:, None] & (row < 0)
        act = np.where(need, self.safe_moves(need), row & 3).astype(np.int8)
        self.v.step(act, self.zeros, want_obs=False)                   # orc_step for the live ones, nothing for the others
        self.t += 1

    def result(self, k0=False):
        """(steps int32 [n], winner int8 [n], codes int8 [n, S, S]) as tron_playout_codes reports them now."""
        v = self.v
        steps = np.where(self.playable, v.eplen, 0).astype(np.int32)
        winner = np.where(self.playable, np.where(v.done == 1, v.winner, -1), -2).astype(np.int8)
        codes = oracle.state_for_player(v.grid, 1).reshape(self.codes.shape)
        codes[~self.playable] = self.codes[~self.playable]
        return steps, winner, (self.codes.copy() if k0 else codes)

    def tally(self):
        """How many playouts are in each of CLASSES now (a playout can be in several)."""
        v, W = self.v, self.W
        fin = self.playable & (v.done == 1)
        pos = v.pos.astype(np.int64)
        same = (pos[:, 0] == pos[:, 2]) & (pos[:, 1] == pos[:, 3])
        off = ((pos < 0) | (pos >= W)).any(1)
        dead_both = (v.alive == 0).all(1)
        counts = (fin & (v.winner == 1), fin & (v.winner == 2), fin & same, fin & dead_both & ~same, fin & off,
                  self.playable & (v.done == 0), self.playable & self.boxed_in, ~self.playable)
        return {k: int(m.sum()) for k, m in zip(CLASSES, counts)}


def playout(codes, actions=None, k_steps=None, ks=None, **key):
    """The model of one tron_playout_codes call, at several k_steps at once: {k: ((steps, winner, codes), tally)} for
    every k in `ks` (default: k_steps alone).  A playout's first k steps do not depend on how many follow."""
    ks = sorted(set([k_steps] if ks is None else ks))
    m = Playouts(codes, **key)
    out = {}
    for t in range(ks[-1] + 1):
        if t in ks:
            out[t] = (m.result(k0=t == 0), m.tally())
        if t < ks[-1] and m.live().any():
            m.step(None if actions is None else actions[t])
        elif t < ks[-1]:
            m.t += 1
    return out


# ---- the inputs of the GPU tests, and of the CPU test that shows they reach every class ------------------------------
SOUP_WIDTHS = (4, 5, 10, 24, 32)
SOUP_N = 1061
SOUP_SEEDS = {4: 11, 5: 12, 10: 13, 24: 14, 32: 15}


def soup_ks(W):
    return (0, 1, 7, W * W)


def soup_boards(W, n=SOUP_N, seed=None):
    """[n, S, S] mid-game boards: the positions of safe-move model games after a random number of steps (0 and up, the
    last live position of a game that ends earlier), with rejected boards mixed in — no +10, two +10, a +10 on the border."""
    rs = np.random.RandomState(SOUP_SEEDS[W] if seed is None else seed)
    S = W + 2
    fresh = np.stack([oracle.state_for_player(oracle.game_init(W, s), 1) for s in start_positions(rs, n, W)])
    length = rs.randint(0, max(2, W * W // 3), n)
    m = Playouts(fresh, seed=rs.randint(1 << 30), stream_id=3, call=rs.randint(1 << 30))
    boards = fresh.copy()
    for t in range(int(length.max())):
        m.step()
        keep = m.live() & (length > t)
        boards[keep] = oracle.state_for_player(m.v.grid[keep], 1).reshape(-1, S, S)
    for i in range(5, n, 53):                                          # rejected boards
        b, kind = boards[i], (i // 53) % 3
        r, c = np.argwhere(b == 10)[0]
        if kind == 0:
            b[r, c] = -2
        elif kind == 1:
            er, ec = np.argwhere(b == 1)[0] if (b == 1).any() else np.argwhere(b == -1)[0]
            b[er, ec] = 10
        else:
            b[r, c] = -2
            b[0, c] = 10
    return boards


def soup_tapes(W, n=SOUP_N, seed=None):
    """{name: int8 [W*W, n, 2] or None}: "full" — bytes over all of 0..127; "none" — every move drawn; "mixed" — even
    playouts: player 1 scripted, player 2 drawn; odd playouts: the first two rows scripted, the rest drawn."""
    rs = np.random.RandomState(1000 + (SOUP_SEEDS[W] if seed is None else seed))
    K = W * W
    full = rs.randint(0, 128, (K, n, 2)).astype(np.int8)
    mixed = rs.randint(0, 128, (K, n, 2)).astype(np.int8)
    drawn = rs.randint(-128, 0, (K, n, 2)).astype(np.int8)
    mixed[:, 0::2, 1] = drawn[:, 0::2, 1]
    mixed[2:, 1::2, :] = drawn[2:, 1::2, :]
    return {"full": full, "none": None, "mixed": mixed}


SOUP_KEY = dict(seed=0xC0FFEE, stream_id=5, call=(7 << 32) | 9)

_soup_cache = {}


def soup(W):
    """(boards, tapes, {tape name: playout(...) at soup_ks(W)}) of width W, computed once per process and never changed."""
    if W not in _soup_cache:
        boards, tapes = soup_boards(W), soup_tapes(W)
        model = {name: playout(boards, tape, ks=soup_ks(W), **SOUP_KEY) for name, tape in tapes.items()}
        _soup_cache[W] = (boards, tapes, model)
    return _soup_cache[W]


# ---- the recorded episodes ---------------------------------------------------------------------------------------------
def suffixes(g):
    """Every suffix of a step-recording fixture as one batch: (boards [m, S, S], tape [K, m, 2], length [m], winner [m],
    final [m, S, S]).  Playout j starts from step_obs1[t], the position after step t of its episode, for every t but the
    episode's last (whose image is a finished game's), and its tape holds the recorded actions after t, padded past the
    episode's end with moves that would go on playing if they were read."""
    off = g["ep_off"].astype(np.int64)
    rs = np.random.RandomState(77)
    rows, eps = [], []
    for e in range(len(off) - 1):
        for t in range(off[e], off[e + 1] - 1):
            rows.append(t)
            eps.append(e)
    rows, eps = np.array(rows), np.array(eps)
    length = off[eps + 1] - 1 - rows
    K = int(length.max()) + 3
    tape = rs.randint(0, 128, (K, len(rows), 2)).astype(np.int8)
    for j, t in enumerate(rows):
        tape[:length[j], j] = g["actions"][t + 1:t + 1 + length[j]]
    return (g["step_obs1"][rows], tape, length.astype(np.int32), g["winner"][eps].astype(np.int8), g["final_obs1"][eps])


def starts(g):
    """The same from every episode's start position: (boards, tape, length, winner, final)."""
    W = int(g["W"])
    off = g["ep_off"].astype(np.int64)
    length = np.diff(off)
    E, K = len(length), int(length.max()) + 3
    boards = np.stack([oracle.state_for_player(oracle.game_init(W, s), 1) for s in g["starts"]])
    tape = np.random.RandomState(78).randint(0, 128, (K, E, 2)).astype(np.int8)
    for e in range(E):
        tape[:length[e], e] = g["actions"][off[e]:off[e + 1]]
    return boards, tape, length.astype(np.int32), g["winner"].astype(np.int8), g["final_obs1"]
