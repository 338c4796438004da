"""The inputs of the weighted-playout tests (tests/test_playout_weighted_model_cpu.py, tests/test_gpu_playout_weighted.py):
the weight vectors, the soups with planted dead ends behind them, the values boards and hand-built boards.  The model is
playout_support's, given weights.  A plain module, imported by name; nothing here needs a GPU."""
import numpy as np

import playout_support as ps
import playout_slide_support as pss
import playout_values_support as pv

UNIFORM_EQUAL = ((1, 1, 1, 1), (0, 0, 0, 0), (7, 7, 7, 7), (255, 255, 255, 255))   # the uniform draw, bit for bit
WEIGHTED = ((1, 8, 4, 2), (0, 255, 0, 1), (3, 0, 0, 0))
WEIGHT_SETS = UNIFORM_EQUAL + WEIGHTED
CANDIDATES = ((1, 8, 4, 2), (1, 4, 2, 1), (0, 4, 2, 1), (1, 1, 2, 4))     # of scripts/playout_policy_match.py: HUG_WEIGHTS is one
DRAW_CLASSES = ps.DRAW_CLASSES


def classes_of(weights):
    """The DRAW_CLASSES a weight vector can meet at all: without a weight of 0 no safe move is ever skipped and the sum is
    never 0.  (With one, a move of any room is still taken where every safe move weighs 0: the fallback.)"""
    return DRAW_CLASSES if 0 in tuple(weights) else tuple(c for c in DRAW_CLASSES if c not in ("zero_skipped", "fallback"))


def packed(weights):
    return sum(int(w) << (8 * k) for k, w in enumerate(weights))


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


def planted_boards(W, n=EXTRA_N, seed=None):
    """[n, S, S] positions of uniform safe-move model games after 0..W-1 steps (the last live one of a game that ends
    earlier); where the head of player 1 (even boards) or 2 (odd boards) has two safe moves or more, one of those that
    lead strictly inside the border is made a dead end: the EMPTY neighbours of its target take the player's trail."""
    rs = np.random.RandomState(EXTRA_SEEDS[W] if seed is None else seed)
    boards = ps.stopped_games(rs, W, n, W, stream_id=4)
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


@ps.once
def soup_boards(W):
    """int8 [N, S, S]: the soup's boards, then the planted ones."""
    return np.concatenate([ps.soup(W)[0], planted_boards(W)])


@ps.once
def soup_tapes_and_rates(W):
    return ps.soup_tapes(W, n=N), pss.soup_rates(W, n=N)


def soup_inputs(W, rule, tape):
    """(boards, rates | None, tape | None) of one GPU case."""
    tapes, rates = soup_tapes_and_rates(W)
    return soup_boards(W), (rates if rule == "slide" else None), tapes[tape]


@ps.once
def soup_model(W, weights, rule, tape):
    """{k: ((steps, winner, codes), tally)} at soup_ks(W) of the N boards of width W under KEY."""
    boards, rates, actions = soup_inputs(W, rule, tape)
    return ps.playout(boards, actions, ks=ps.soup_ks(W), rates=rates, weights=weights, **KEY)


def values_boards(W):
    return pv.boards(W)


def values_rates(W):
    return pss.soup_rates(W)[list(pv.SELECT)]


@ps.once
def values_soup_model(W, weights, rule, copies):
    """{k: (counts, steps, actions)} of playout_values_support's 38 boards of width W at its ks(W) under KEY."""
    rates = values_rates(W) if rule == "slide" else None
    return ps.values_model(values_boards(W), None, copies, ks=pv.ks(W), rates=rates, weights=weights, **KEY)


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
