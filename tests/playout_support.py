"""What the playout tests share: the one host model of the tron_playout_* entries, built on the CPU oracle, and the plain
soup's boards and tapes (the per-feature inputs are in playout_slide_support, playout_values_support,
playout_weighted_support and territory_support, which hold inputs only).  The model decodes player 1's code images to
Tile grids and head positions, steps them with the oracle's orc_step (through VecOracle, whose arrays it fills), encodes
with state_for_player, and draws safe moves from the oracle's Philox as include/tron_hip.h states them.  Two independent
choices make the four entries' models:
  rates    None steps a VecOracle in mode None.  float64 [n, 2] steps one in mode "ice" whose every env slides at 0.5: per
           step the model decides `float64(u) <= rate` per (playout, player) in numpy and hands orc_step the uniform 0.25
           where that holds and 0.75 where not.  orc_step consumes a uniform only on an in-bounds empty target, so this is
           the rule of include/tron_hip.h for any per-player rates, and the rule itself stays in the oracle.  u is the
           caller's tape, or words 2 and 3 of the Philox block whose words 0 and 1 are the safe draws.
  weights  None draws uniformly by the rank of a candidate; four weights draw by weighted_pick, written in coordinates
           with a uniform fallback of its own.
A plain module, imported by name; nothing here needs a GPU."""
import ctypes as C
import functools

import numpy as np

import oracle
from rollout_support import start_positions

EMPTY, WALL, P1_BODY, P1_HEAD, P2_BODY, P2_HEAD = 0, -1, 1, 2, 3, 4      # raw tile values (map.py:9-17)
CLASSES = ("p1_wins", "p2_wins", "same_cell", "both_crash", "border_deaths", "unfinished", "boxed_in", "rejected")
SLIDE_CLASSES = ("slide", "both_slid", "slide_to_border", "slide_to_trail", "p2_target_filled", "p1_dies_on_p2_tile")
# what a drawn move can be: the room of the move taken; a safe move of weight 0 beside one that weighs something; all safe
# moves of weight 0, two or more of them; no safe move; a move other than the uniform draw's at the same u
DRAW_CLASSES = ("room0", "room1", "room2", "room3", "zero_skipped", "fallback", "no_candidate", "not_uniform")
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


def philox_uniform(word):
    """The env's conversion of a Philox word to a slide uniform: (word >> 8) * 2^-24, a float32."""
    return (np.asarray(word, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def weighted_pick(w, free, u):
    """The weighted draw's steps 1 and 2 for arrays [..., 4] in UP, RIGHT, DOWN, LEFT order: w the weight of each
    direction's room (looked at where `free`), u the Philox word [...].  Returns (move, T, cnt)."""
    free = np.asarray(free, bool)
    w = np.where(free, np.asarray(w, np.uint64), np.uint64(0))
    u = np.asarray(u, np.uint64)
    cnt = free.sum(-1)
    T = w.sum(-1)
    x = (u * T) >> np.uint64(32)                                       # mulhi(u, T), < T
    weighted = (np.cumsum(w, -1) > x[..., None]).argmax(-1)            # the first whose running sum exceeds x
    j = (u * cnt.astype(np.uint64)) >> np.uint64(32)                   # mulhi(u, cnt): the uniform rule
    uniform = (free & (np.cumsum(free, -1) - 1 == j[..., None].astype(np.int64))).argmax(-1)
    return np.where(T > 0, weighted, np.where(cnt > 0, uniform, 0)), T, cnt


class Playouts:
    """n boards stepped together under the rule `rates` and the draw `weights` choose (see the module's docstring);
    uniforms: float32 [K, n, 2] or None (Philox), with rates only.  step(row) plays one step of every playout that is
    still live: row int8 [n, 2], a byte 0..127 an action (its low two bits), a negative byte a safe draw."""

    def __init__(self, codes, rates=None, uniforms=None, weights=None, seed=0x5EED, stream_id=0, call=0, first_index=0):
        assert rates is not None or uniforms is None
        self.codes = np.ascontiguousarray(codes, np.int8)
        self.n, self.S = self.codes.shape[0], self.codes.shape[-1]
        self.W = self.S - 2
        tiles, pos, self.playable = decode(self.codes)
        self.v = v = oracle.VecOracle(self.n, self.W, mode=None) if rates is None else \
            oracle.VecOracle(self.n, self.W, mode="ice", slide=0.5)
        v.grid[:], v.pos[:], v.done[:] = tiles, pos, ~self.playable
        self.philox = _Philox(seed, stream_id, call)
        self.first_index = first_index                                 # playout i is index first_index + i of its launch
        self.t = 0
        self.boxed_in = np.zeros(self.n, bool)                         # a safe draw found no candidate
        self.zeros = np.zeros((self.n, 2), np.float32)
        self.rates = None if rates is None else np.ascontiguousarray(rates, np.float64).reshape(self.n, 2)
        self.uniforms = None if uniforms is None else np.ascontiguousarray(uniforms, np.float32)
        if rates is not None:
            self.can_slide = self.rates >= 0                           # under a drawn u, which is >= 0 (NaN: False)
            self.seen = dict.fromkeys(SLIDE_CLASSES, 0)                # steps of this call in each class, so far
        self.weights = None if weights is None else np.array(weights, np.uint64)
        if weights is not None:
            assert self.weights.shape == (4,) and (self.weights <= 255).all()
            self.drawn = dict.fromkeys(DRAW_CLASSES, 0)                # drawn moves of live playouts in each class, so far

    def live(self):
        return self.v.done == 0

    def words(self, rows):
        """uint64 [m, 2]: words 0 and 1 of this step's Philox block of each playout in `rows`."""
        return np.array([self.philox.words(self.first_index + i, self.t)[:2].copy() for i in rows], np.uint64)

    def safe_moves(self, need):
        """[n, 2] the safe draw of every (playout, player) in `need`, 0 elsewhere."""
        out = np.zeros((self.n, 2), np.int8)
        rows = np.nonzero(need.any(1))[0]
        if len(rows):
            nd = need[rows]
            move, cnt = self.uniform_moves(rows) if self.weights is None else self.weighted_moves(rows, nd)
            out[rows] = np.where(nd, move, 0)
            self.boxed_in[rows] |= (nd & (cnt == 0)).any(1)
        return out

    def uniform_moves(self, rows):
        """(move [m, 2], candidates [m, 2]) of the uniform draw: the candidate whose rank is mulhi(u, candidates)."""
        v, S = self.v, self.S
        pos = v.pos[rows].astype(np.int64).reshape(-1, 2, 2)           # [m, player, (r, c)]
        cell = (pos[:, :, 0] + 1) * S + (pos[:, :, 1] + 1)
        target = cell[:, :, None] + (DR * S + DC)[None, None, :]       # [m, 2, 4] in UP, RIGHT, DOWN, LEFT order
        free = v.grid[rows[:, None, None], target] == EMPTY            # the board as it stands: a head is no empty cell
        cnt = free.sum(2)
        pick = (self.words(rows) * cnt.astype(np.uint64)) >> np.uint64(32)      # mulhi(u, c)
        rank = np.cumsum(free, 2) - 1                                  # a candidate's place in the list
        return (free & (rank == pick[:, :, None].astype(np.int64))).argmax(2), cnt   # none: argmax of all False = 0 = UP

    def rooms(self, rows):
        """(free bool [m, 2, 4], room int [m, 2, 4]) of players' four moves on the board as it stands: the EMPTY cells
        among the target's three neighbours other than the mover's head; a cell outside the image is not EMPTY."""
        v, S = self.v, self.S
        grid = v.grid[rows].reshape(len(rows), S, S)
        pos = v.pos[rows].astype(np.int64).reshape(-1, 2, 2) + 1        # [m, player, (r, c)] in the padded image
        take = np.arange(len(rows))[:, None, None]
        tr, tc = pos[:, :, 0, None] + DR, pos[:, :, 1, None] + DC      # [m, 2, 4]
        free = grid[take, tr, tc] == EMPTY                             # a head is strictly inside: its targets are cells
        room = np.zeros(free.shape, np.int64)
        for b in range(4):
            nr, nc = tr + DR[b], tc + DC[b]
            inside = (nr >= 0) & (nc >= 0) & (nr < S) & (nc < S)
            back = (np.arange(4) ^ 2) == b                             # direction b from the target of a leads to the head
            cell = grid[take, np.clip(nr, 0, S - 1), np.clip(nc, 0, S - 1)]
            room += inside & ~back & (cell == EMPTY)
        return free, room

    def weighted_moves(self, rows, nd):
        """(move, candidates) of the weighted draw; counts the drawn ones, `nd`, per DRAW_CLASSES."""
        free, room = self.rooms(rows)
        u = self.words(rows)
        move, T, cnt = weighted_pick(self.weights[room], free, u)
        plain = weighted_pick(np.ones(4, np.uint64), free, u)[0]
        taken = np.take_along_axis(room, move[:, :, None], 2)[:, :, 0]
        zero = (free & (self.weights[room] == 0)).any(2)
        for k in range(4):
            self.drawn[f"room{k}"] += int((nd & (cnt > 0) & (taken == k)).sum())
        self.drawn["zero_skipped"] += int((nd & (T > 0) & zero).sum())
        self.drawn["fallback"] += int((nd & (T == 0) & (cnt >= 2)).sum())
        self.drawn["no_candidate"] += int((nd & (cnt == 0)).sum())
        self.drawn["not_uniform"] += int((nd & (move != plain)).sum())
        return move, cnt

    def slides(self, live):
        """bool [n, 2]: float64(u) <= rate of this step, for the live playouts (False elsewhere)."""
        if self.uniforms is not None:
            u = self.uniforms[self.t]
        else:
            u = np.ones((self.n, 2), np.float32)
            for i in np.nonzero(live & self.can_slide.any(1))[0]:      # a drawn u is >= 0: it meets no other rate
                u[i] = philox_uniform(self.philox.words(self.first_index + i, self.t)[2:])
        with np.errstate(invalid="ignore"):
            return live[:, None] & (u.astype(np.float64) <= self.rates)

    def classify(self, live, act, slides):
        """Counts this step's playouts per SLIDE_CLASSES from the position before it (orc_step decides the step itself)."""
        v, S, W = self.v, self.S, self.W
        rows = np.nonzero(live)[0]
        if not len(rows):
            return
        pos = v.pos[rows].astype(np.int64).reshape(-1, 2, 2)
        a = act[rows].astype(np.int64) & 3
        dr, dc = DR[a], DC[a]
        nr, nc = pos[:, :, 0] + dr, pos[:, :, 1] + dc                  # the targets
        inside = (nr >= 0) & (nc >= 0) & (nr < W) & (nc < W)
        n = (nr + 1) * S + (nc + 1)
        grid = v.grid[rows]
        take = np.arange(len(rows))[:, None]
        empty = inside & (grid[take, n] == EMPTY)                      # (a head's cell is no empty cell)
        want = slides[rows]
        slid0 = empty[:, 0] & want[:, 0]
        filled = empty[:, 1] & slid0 & (n[:, 1] == n[:, 0])
        slid1 = empty[:, 1] & ~filled & want[:, 1]
        slid = np.stack([slid0, slid1], 1)
        lr, lc = nr + dr * slid, nc + dc * slid                        # where the heads land
        f = (lr + 1) * S + (lc + 1)
        landed_inside = (lr >= 0) & (lc >= 0) & (lr < W) & (lc < W)
        other_tile = np.stack([slid1 & (f[:, 0] == n[:, 1]), slid0 & (f[:, 1] == n[:, 0])], 1)
        on_trail = slid & landed_inside & ((grid[take, np.clip(f, 0, S * S - 1)] != EMPTY) | other_tile)
        for name, m in (("slide", slid.any(1)), ("both_slid", slid.all(1)), ("slide_to_border", (slid & ~landed_inside).any(1)),
                        ("slide_to_trail", on_trail.any(1)), ("p2_target_filled", filled),
                        ("p1_dies_on_p2_tile", slid1 & (f[:, 0] == n[:, 1]))):
            self.seen[name] += int(m.sum())

    def step(self, row=None):
        live = self.live()
        row = np.full((self.n, 2), -1, np.int8) if row is None else np.asarray(row, np.int8)
        need = live[:, None] & (row < 0)
        act = np.where(need, self.safe_moves(need), row & 3).astype(np.int8)
        u = self.zeros
        if self.rates is not None:
            slides = self.slides(live)
            self.classify(live, act, slides)
            u = np.where(slides, np.float32(0.25), np.float32(0.75))
        self.v.step(act, u, want_obs=False)                            # orc_step for the live ones, nothing for the others
        self.t += 1

    def result(self, k0=False):
        """(steps int32 [n], winner int8 [n], codes int8 [n, S, S]) as the entries report them now."""
        v = self.v
        steps = np.where(self.playable, v.eplen, 0).astype(np.int32)
        winner = np.where(self.playable, np.where(v.done == 1, v.winner, -1), -2).astype(np.int8)
        codes = oracle.state_for_player(v.grid, 1).reshape(self.codes.shape)
        codes[~self.playable] = self.codes[~self.playable]
        return steps, winner, (self.codes.copy() if k0 else codes)

    def tally(self):
        """How many playouts are in each of CLASSES now (a playout can be in several); under weights the drawn moves so
        far per DRAW_CLASSES and under rates the steps so far per SLIDE_CLASSES before them."""
        v, W = self.v, self.W
        fin = self.playable & (v.done == 1)
        pos = v.pos.astype(np.int64)
        same = (pos[:, 0] == pos[:, 2]) & (pos[:, 1] == pos[:, 3])
        off = ((pos < 0) | (pos >= W)).any(1)
        dead_both = (v.alive == 0).all(1)
        counts = (fin & (v.winner == 1), fin & (v.winner == 2), fin & same, fin & dead_both & ~same, fin & off,
                  self.playable & (v.done == 0), self.playable & self.boxed_in, ~self.playable)
        out = {} if self.weights is None else dict(self.drawn)
        if self.rates is not None:
            out.update(self.seen)
        out.update((k, int(m.sum())) for k, m in zip(CLASSES, counts))
        return out


def playout(codes, actions=None, k_steps=None, ks=None, rates=None, uniforms=None, weights=None, **key):
    """The model of one call of tron_playout_codes (rates and weights None), tron_playout_slide_codes (rates),
    tron_playout_weighted_codes (weights, under either rule), at several k_steps at once: {k: ((steps, winner, codes),
    tally)} for every k in `ks` (default: k_steps alone).  A playout's first k steps do not depend on how many follow."""
    ks = sorted(set([k_steps] if ks is None else ks))
    m = Playouts(codes, rates, uniforms, weights, **key)
    out = {}
    for t in range(ks[-1] + 1):
        if t in ks:
            out[t] = (m.result(k0=t == 0), m.tally())
        if t < ks[-1] and m.live().any():
            m.step(None if actions is None else actions[t])
        elif t < ks[-1]:
            m.t += 1
    return out


# ---- tron_playout_values and its kin: defined through the codes entries, so their model is a composition of playout ----
def fan_out(codes, k_steps, copies):
    """The launch tron_playout_values stands for: (boards [n * 16 * copies, S, S], tape int8 [k_steps, n * 16 * copies, 2]).
    Index q = ((i * 16 + a1 * 4 + a2) * copies + j) holds board i; the tape's row 0 holds (a1, a2), every other row is
    negative (safe draws)."""
    codes = np.ascontiguousarray(codes, np.int8)
    n = len(codes)
    boards = np.repeat(codes, 16 * copies, axis=0)
    tape = np.full((k_steps, n * 16 * copies, 2), -1, np.int8)
    if k_steps:
        move = (np.arange(n * 16 * copies) // copies) % 16
        tape[0, :, 0], tape[0, :, 1] = move >> 2, move & 3
    return boards, tape


def tally(steps, winner, n, copies):
    """(counts int32 [n, 4, 4, 4], steps int32 [n, 4, 4]) of one fanned-out launch's out_steps and out_winner."""
    q = np.arange(n * 16 * copies)
    board, move = q // (16 * copies), (q // copies) % 16
    counts = np.zeros((n, 4, 4, 4), np.int32)
    total = np.zeros((n, 4, 4), np.int32)
    played = winner != -2
    np.add.at(counts, (board[played], move[played] >> 2, move[played] & 3, winner[played].astype(np.int64) & 3), 1)   # -1 -> 3
    np.add.at(total, (board, move >> 2, move & 3), steps)              # a rejected board's steps are 0
    return counts, total


def pick(counts):
    """int8 [n, 2]: each player's maximin move on m = wins of 1 - wins of 2 (negated for player 2): the first move in UP,
    RIGHT, DOWN, LEFT order whose worst case over the opponent's four moves is greatest; -1 where nothing was played."""
    counts = np.asarray(counts).astype(np.int64)
    m = counts[..., 1] - counts[..., 2]                                # [n, a1, a2]
    act = np.stack([m.min(2).argmax(1), (-m).min(1).argmax(1)], 1).astype(np.int8)
    act[counts.reshape(len(counts), -1).sum(1) == 0] = -1
    return act


def values_model(codes, k_steps, copies, ks=None, rates=None, weights=None, **key):
    """The model of one tron_playout_values / _slide_values / _weighted_values call: playout on the fanned-out launch
    (board i's rates row for all its playouts), tallied.  (counts, steps, actions); with `ks` {k: that triple} at several
    k_steps at once."""
    many = sorted(set([k_steps] if ks is None else ks))
    n = len(codes)
    boards, tape = fan_out(codes, many[-1], copies)
    fanned = None if rates is None else np.repeat(np.asarray(rates, np.float64), 16 * copies, axis=0)
    out = {}
    for k, ((steps, winner, _), _) in playout(boards, tape, ks=many, rates=fanned, weights=weights, **key).items():
        counts, total = tally(steps, winner, n, copies)
        out[k] = (counts, total, pick(counts))
    return out if ks is not None else out[k_steps]


# ---- what every input module shares: the one cache, and model games stopped early -------------------------------------
_cache = {}


def once(make):
    """make(*args, **kw) computed once per process and per arguments, and never changed: the one cache of these tests."""
    @functools.wraps(make)
    def get(*args, **kw):
        at = (make.__module__, make.__name__, args, tuple(sorted(kw.items())))
        if at not in _cache:
            _cache[at] = make(*args, **kw)
        return _cache[at]
    return get


def stopped_games(rs, W, n, longest, stream_id):
    """[n, S, S] the positions of uniform safe-move model games from random starts after a random number of steps, 0 to
    longest - 1 (the last live position of a game that ends earlier), everything drawn from the RandomState `rs`."""
    S = W + 2
    fresh = np.stack([oracle.state_for_player(oracle.game_init(W, s), 1) for s in start_positions(rs, n, W)])
    length = rs.randint(0, longest, n)
    m = Playouts(fresh, seed=rs.randint(1 << 30), stream_id=stream_id, call=rs.randint(1 << 30))
    boards = fresh.copy()
    for t in range(int(length.max())):
        m.step()
        keep = m.live() & (length > t)
        boards[keep] = oracle.state_for_player(m.v.grid[keep], 1).reshape(-1, S, S)
    return boards


def spoil_some(boards):
    """Makes every 53rd board from the 5th one that the entries reject, in turn: no +10, two +10, a +10 on the border."""
    for i in range(5, len(boards), 53):
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
    return spoil_some(stopped_games(rs, W, n, max(2, W * W // 3), stream_id=3))


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



@once
def soup(W):
    """(boards, tapes, {tape name: playout(...) at soup_ks(W)}) of width W."""
    boards, tapes = soup_boards(W), soup_tapes(W)
    return boards, tapes, {name: playout(boards, tape, ks=soup_ks(W), **SOUP_KEY) for name, tape in tapes.items()}


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
