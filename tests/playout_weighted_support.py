"""What the weighted-playout tests share (tests/test_playout_weighted_model_cpu.py, tests/test_gpu_playout_weighted.py): the
host model of tron_playout_weighted_codes / tron_playout_weighted_values and the inputs both files use.  The model is
playout_support.Playouts (mode None's rule) or playout_slide_support.SlidePlayouts (the sliding rule) with safe_moves
alone replaced by the weighted draw of include/tron_hip.h, written here in coordinates: the step stays the oracle's
orc_step, the slide decision stays SlidePlayouts'.  A plain module, imported by name; nothing here needs a GPU."""
import numpy as np

import oracle
import playout_support as ps
import playout_slide_support as pss
import playout_values_support as pv
from rollout_support import start_positions

UNIFORM_EQUAL = ((1, 1, 1, 1), (0, 0, 0, 0), (7, 7, 7, 7), (255, 255, 255, 255))   # the uniform draw, bit for bit
WEIGHTED = ((1, 8, 4, 2), (0, 255, 0, 1), (3, 0, 0, 0))
WEIGHT_SETS = UNIFORM_EQUAL + WEIGHTED
CANDIDATES = ((1, 8, 4, 2), (1, 4, 2, 1), (0, 4, 2, 1), (1, 1, 2, 4))     # of scripts/playout_policy_match.py: HUG_WEIGHTS is one
# what a drawn move can be: the room of the move taken; a safe move of weight 0 beside one that weighs something; all safe
# moves of weight 0, two or more of them; no safe move; a move other than the uniform draw's at the same u
DRAW_CLASSES = ("room0", "room1", "room2", "room3", "zero_skipped", "fallback", "no_candidate", "not_uniform")


def classes_of(weights):
    """The DRAW_CLASSES a weight vector can meet at all: without a weight of 0 no safe move is ever skipped and the sum is
    never 0.  (With one, a move of any room is still taken where every safe move weighs 0: the fallback.)"""
    return DRAW_CLASSES if 0 in tuple(weights) else tuple(c for c in DRAW_CLASSES if c not in ("zero_skipped", "fallback"))


def packed(weights):
    return sum(int(w) << (8 * k) for k, w in enumerate(weights))


def pick(w, free, u):
    """The rule's steps 1 and 2 for arrays [..., 4] in UP, RIGHT, DOWN, LEFT order: w the weight of each direction's room
    (looked at where `free`), u the Philox word [...].  Returns (move, T, cnt)."""
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


class _Weighted:
    """safe_moves under four weights; `drawn` counts the drawn moves of live playouts per DRAW_CLASSES."""

    def set_weights(self, weights):
        self.weights = np.array(weights, np.uint64)
        assert self.weights.shape == (4,) and (self.weights <= 255).all()
        self.drawn = dict.fromkeys(DRAW_CLASSES, 0)

    def rooms(self, rows):
        """(free bool [m, 2, 4], room int [m, 2, 4]) of players' four moves on the board as it stands: the EMPTY cells
        among the target's three neighbours other than the mover's head; a cell outside the image is not EMPTY."""
        v, S = self.v, self.S
        grid = v.grid[rows].reshape(len(rows), S, S)
        pos = v.pos[rows].astype(np.int64).reshape(-1, 2, 2) + 1        # [m, player, (r, c)] in the padded image
        take = np.arange(len(rows))[:, None, None]
        tr, tc = pos[:, :, 0, None] + ps.DR, pos[:, :, 1, None] + ps.DC  # [m, 2, 4]
        free = grid[take, tr, tc] == ps.EMPTY                          # a head is strictly inside: its targets are cells
        room = np.zeros(free.shape, np.int64)
        for b in range(4):
            nr, nc = tr + ps.DR[b], tc + ps.DC[b]
            inside = (nr >= 0) & (nc >= 0) & (nr < S) & (nc < S)
            back = (np.arange(4) ^ 2) == b                             # direction b from the target of a leads to the head
            cell = grid[take, np.clip(nr, 0, S - 1), np.clip(nc, 0, S - 1)]
            room += inside & ~back & (cell == ps.EMPTY)
        return free, room

    def safe_moves(self, need):
        out = np.zeros((self.n, 2), np.int8)
        rows = np.nonzero(need.any(1))[0]
        if not len(rows):
            return out
        free, room = self.rooms(rows)
        u = np.array([self.philox.words(self.first_index + i, self.t)[:2].copy() for i in rows], np.uint64)
        move, T, cnt = pick(self.weights[room], free, u)
        plain = pick(np.ones(4, np.uint64), free, u)[0]
        out[rows] = np.where(need[rows], move, 0)
        self.boxed_in[rows] |= (need[rows] & (cnt == 0)).any(1)
        nd = need[rows]
        taken = np.take_along_axis(room, move[:, :, None], 2)[:, :, 0]
        zero = (free & (self.weights[room] == 0)).any(2)
        for k in range(4):
            self.drawn[f"room{k}"] += int((nd & (cnt > 0) & (taken == k)).sum())
        self.drawn["zero_skipped"] += int((nd & (T > 0) & zero).sum())
        self.drawn["fallback"] += int((nd & (T == 0) & (cnt >= 2)).sum())
        self.drawn["no_candidate"] += int((nd & (cnt == 0)).sum())
        self.drawn["not_uniform"] += int((nd & (move != plain)).sum())
        return out

    def tally(self):
        return dict(self.drawn, **super().tally())


class WeightedPlayouts(_Weighted, ps.Playouts):
    def __init__(self, codes, weights, **key):
        super().__init__(codes, **key)
        self.set_weights(weights)


class WeightedSlidePlayouts(_Weighted, pss.SlidePlayouts):
    def __init__(self, codes, weights, rates, uniforms=None, **key):
        super().__init__(codes, rates, uniforms, **key)
        self.set_weights(weights)


def playout(codes, weights, rates=None, actions=None, uniforms=None, k_steps=None, ks=None, **key):
    """The model of one tron_playout_weighted_codes call, at several k_steps at once: {k: ((steps, winner, codes), tally)}
    for every k in `ks` (default: k_steps alone), as playout_support.playout.  rates=None: mode None's rule."""
    assert rates is not None or uniforms is None
    ks = sorted(set([k_steps] if ks is None else ks))
    m = WeightedPlayouts(codes, weights, **key) if rates is None else WeightedSlidePlayouts(codes, weights, rates, uniforms, **key)
    out = {}
    for t in range(ks[-1] + 1):
        if t in ks:
            out[t] = (m.result(k0=t == 0), m.tally())
        if t < ks[-1] and m.live().any():
            m.step(None if actions is None else actions[t])
        elif t < ks[-1]:
            m.t += 1
    return out


def values_model(codes, weights, k_steps, copies, rates=None, ks=None, **key):
    """The model of one tron_playout_weighted_values call, built as playout_values_support.values_model is: the weighted
    codes model on the fanned-out launch (board i's rates row for all its playouts), tallied.  (counts, steps, actions),
    or with `ks` {k: that triple}."""
    many = sorted(set([k_steps] if ks is None else ks))
    n = len(codes)
    boards, tape = pv.fan_out(codes, many[-1], copies)
    fanned = None if rates is None else np.repeat(np.asarray(rates, np.float64), 16 * copies, axis=0)
    out = {}
    for k, ((steps, winner, _), _) in playout(boards, weights, fanned, tape, ks=many, **key).items():
        counts, total = pv.tally(steps, winner, n, copies)
        out[k] = (counts, total, pv.pick(counts))
    return out if ks is not None else out[k_steps]


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------
# playout_support's 1 061 soup boards of a width and, behind them, EXTRA_N early positions with a dead end planted beside
# one head.  The soup's boards are mostly last live positions, where a weighted draw rarely has a choice that matters (at
# width 32 the (3,0,0,0) model departs from the uniform one on 4 % of them); with the planted boards every non-uniform
# weight vector departs on more than one board in ten at every width and under either rule, which
# tests/test_playout_weighted_model_cpu.py pins.  Rates and tapes are playout_slide_support's and playout_support's at N.
WIDTHS = (4, 5, 10, 32)
EXTRA_N = 512
N = ps.SOUP_N + EXTRA_N
EXTRA_SEEDS = {4: 74, 5: 75, 10: 80, 32: 102}
KEY = dict(seed=0xB0A7, stream_id=6, call=(2 << 32) | 27)
TAPES = ("none", "mixed")
RULES = ("plain", "slide")

_cache = {}


def planted_boards(W, n=EXTRA_N, seed=None):
    """[n, S, S] positions of uniform safe-move model games after 0..W-1 steps (the last live one of a game that ends
    earlier); where the head of player 1 (even boards) or 2 (odd boards) has two safe moves or more, one of those that
    lead strictly inside the border is made a dead end: the EMPTY neighbours of its target take the player's trail."""
    rs = np.random.RandomState(EXTRA_SEEDS[W] if seed is None else seed)
    S = W + 2
    fresh = np.stack([oracle.state_for_player(oracle.game_init(W, s), 1) for s in start_positions(rs, n, W)])
    length = rs.randint(0, W, n)
    m = ps.Playouts(fresh, seed=rs.randint(1 << 30), stream_id=4, call=rs.randint(1 << 30))
    boards = fresh.copy()
    for t in range(int(length.max())):
        m.step()
        keep = m.live() & (length > t)
        boards[keep] = oracle.state_for_player(m.v.grid[keep], 1).reshape(-1, S, S)
    for i, b in enumerate(boards):
        head, trail = (10, -2) if i % 2 == 0 else (-10, -3)
        r, c = np.argwhere(b == head)[0]
        free = [a for a in range(4) if b[r + ps.DR[a], c + ps.DC[a]] == 1]
        inner = [a for a in free if 1 <= r + ps.DR[a] <= W and 1 <= c + ps.DC[a] <= W]
        if len(free) < 2 or not inner:
            continue
        a = inner[rs.randint(len(inner))]
        for d in range(4):
            nr, nc = r + ps.DR[a] + ps.DR[d], c + ps.DC[a] + ps.DC[d]
            if b[nr, nc] == 1:
                b[nr, nc] = trail
    return boards


def soup_boards(W):
    """int8 [N, S, S]: the soup's boards, then the planted ones; computed once per process and never changed."""
    if ("boards", W) not in _cache:
        _cache["boards", W] = np.concatenate([ps.soup(W)[0], planted_boards(W)])
    return _cache["boards", W]


def soup_inputs(W, rule, tape):
    """(boards, rates | None, tape | None) of one GPU case."""
    if ("tapes", W) not in _cache:
        _cache["tapes", W] = (ps.soup_tapes(W, n=N), pss.soup_rates(W, n=N))
    tapes, rates = _cache["tapes", W]
    return soup_boards(W), (rates if rule == "slide" else None), tapes[tape]


def soup_model(W, weights, rule, tape):
    """{k: ((steps, winner, codes), tally)} at soup_ks(W) of the N boards of width W under KEY, computed once per process
    and never changed."""
    at = (W, tuple(weights), rule, tape)
    if at not in _cache:
        boards, rates, actions = soup_inputs(W, rule, tape)
        _cache[at] = playout(boards, weights, rates, actions, ks=ps.soup_ks(W), **KEY)
    return _cache[at]


def values_boards(W):
    return pv.boards(W)


def values_rates(W):
    return pss.soup_rates(W)[list(pv.SELECT)]


def values_soup_model(W, weights, rule, copies):
    """{k: (counts, steps, actions)} of playout_values_support's 38 boards of width W at its ks(W) under KEY."""
    at = ("values", W, tuple(weights), rule, copies)
    if at not in _cache:
        rates = values_rates(W) if rule == "slide" else None
        _cache[at] = values_model(values_boards(W), weights, None, copies, rates, ks=pv.ks(W), **KEY)
    return _cache[at]


# ---- hand-built boards: a head with two safe moves, one into a dead end and one into the open --------------------------
UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3


def _fresh(W):
    b = np.ones((W + 2, W + 2), np.int8)
    b[0], b[-1], b[:, 0], b[:, -1] = -1, -1, -1, -1
    return b


def _orientations(board):
    """The eight images of a board under the square's symmetries."""
    out = []
    for flip in (False, True):
        b = board.T if flip else board
        out += [np.rot90(b, q) for q in range(4)]
    return out


def _move_between(board, head, target):
    (r0, c0), (r1, c1) = np.argwhere(board == head)[0], np.argwhere(board == target)[0]
    return {(-1, 0): UP, (0, 1): RIGHT, (1, 0): DOWN, (0, -1): LEFT}[(r1 - r0, c1 - c0)]


def dead_end_boards():
    """(boards int8 [m, 9, 9], player [m], dead-end move [m], open move [m]): on a 7x7 board one player's head has exactly
    two safe moves — one onto a cell of room 0 (walled in on its three other sides), one onto a cell of room 3 — for
    either player, in all eight orientations.  The other player sits in a far corner with safe moves of its own."""
    W = 7
    base = _fresh(W)
    # the head at (4, 4) of the padded image.  (3, 4) above it is the dead end: (2, 4), (3, 3), (3, 5) are trail.  (5, 4)
    # below it is the open cell: (6, 4), (5, 3), (5, 5) are EMPTY.  (4, 3) and (4, 5) beside it are trail: not safe.
    base[4, 4] = 10
    for r, c in ((2, 4), (3, 3), (3, 5), (4, 3), (4, 5)):
        base[r, c] = -2
    base[1, 1] = -10
    marks = base.copy()                                                # 20: the dead end, 30: the open cell
    marks[3, 4], marks[5, 4] = 20, 30
    boards, player, dead, opened = [], [], [], []
    for b, m in zip(_orientations(base), _orientations(marks)):
        for p in (1, 2):
            img = np.ascontiguousarray(b).copy()
            if p == 2:                                                 # swap the two players: heads and trails
                img = np.select([b == 10, b == -10, b == -2, b == -3], [-10, 10, -3, -2], b).astype(np.int8)
            boards.append(img)
            player.append(p)
            dead.append(_move_between(m, 10, 20))
            opened.append(_move_between(m, 10, 30))
    return np.stack(boards), np.array(player), np.array(dead), np.array(opened)


def border_boards():
    """int8 [m, 6, 6]: the same head on a 4x4 board in each corner and against each border, where the targets that are
    not safe are border cells whose neighbours lie off the image; and one board whose border holds EMPTY cells (no env
    makes one), where a target on the border ring is a candidate whose off-image neighbour is not EMPTY."""
    W = 4
    boards = []
    for r in range(1, W + 1):
        for c in range(1, W + 1):
            if 1 < r < W and 1 < c < W:
                continue                                               # interior: dead_end_boards' ground
            b = _fresh(W)
            b[r, c] = 10
            far_r, far_c = (W if r <= W // 2 else 1), (W if c <= W // 2 else 1)
            b[far_r, far_c] = -10
            if r + 1 <= W and (r + 1, c) != (far_r, far_c):
                for rr, cc in ((r + 2, c), (r + 1, c - 1), (r + 1, c + 1)):   # wall the cell below the head in: room 0
                    if 1 <= rr <= W and 1 <= cc <= W and b[rr, cc] == 1:
                        b[rr, cc] = -3
            boards.append(b)
    leaky = _fresh(W)
    leaky[1, 1], leaky[4, 4] = 10, -10
    leaky[0, :], leaky[:, 0] = 1, 1                                    # EMPTY on the border ring
    boards.append(leaky)
    boards.append(leaky[::-1, ::-1].copy())
    return np.stack(boards)
