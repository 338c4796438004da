"""What the reach tests share (tests/test_reach_model_cpu.py, tests/test_gpu_reach.py): a vectorised numpy model of
tron_reach_codes as include/tron_hip.h defines it, built on territory_support's flood; a literal one-board queue BFS written
independently of it; the wrong models that the inputs must tell from the right one; the hand boards and the planted boards.
The soups, the early and the planted boards of territory_support are the inputs here too.  A plain module, imported by name;
nothing here needs a GPU."""
import numpy as np

import playout_support as ps
import territory_support as terr

OPP1, SAME1, OPP2, SAME2, FILL1, FILL2, DEPTH1, DEPTH2 = range(8)
SIDES = (6, 8, 9, 16, 17, 32, 33, 34)


# ---- the model -----------------------------------------------------------------------------------------------------------
def model(codes, absolute_colour=False, swapped_fill=False, always_plus_one=False, reach_as_first=False,
          head_minus_one=False, through_head=False, saturate=None, depth_over_first=False):
    """(counts int32 [n, 8], dist int16 [n, 2, S, S]) of a stack of player-1 code boards.  The keywords are the WRONG models."""
    codes = np.ascontiguousarray(codes, np.int8)
    n, S = codes.shape[0], codes.shape[-1]
    inner = np.zeros((S, S), bool)
    inner[1:-1, 1:-1] = True
    playable = (terr.model(codes)[0][:, 0] >= 0)[:, None, None]
    open_ = (codes == 1) & inner & playable
    heads = [(codes == 10) & playable, (codes == -10) & playable]
    colour = (np.add.outer(np.arange(S), np.arange(S)) & 1)[None]
    d, fin = [], []
    for p in range(2):
        passable = open_ | heads[1 - p] if through_head else open_
        dp = terr._flood(passable, heads[p])
        if saturate is not None:
            dp = np.where(dp < terr.INF, np.minimum(dp, saturate), dp)
        d.append(dp)
        fin.append(dp < terr.INF)
    counts = np.zeros((n, 8), np.int32)
    dist = np.full((n, 2, S, S), -1, np.int16)
    for p in range(2):
        q = 1 - p
        first = open_ & fin[p] if reach_as_first else open_ & fin[p] & (~fin[q] | (d[p] < d[q]))
        head_colour = np.zeros((n, 1, 1), np.int64) if absolute_colour else (colour * heads[p]).sum((1, 2))[:, None, None]
        same = (first & (colour == head_colour)).sum((1, 2))
        opp = first.sum((1, 2)) - same
        if swapped_fill:
            fill = np.where(same > opp, 2 * opp + 1, 2 * same)
        elif always_plus_one:
            fill = 2 * np.minimum(opp, same) + 1
        else:
            fill = np.where(opp > same, 2 * same + 1, 2 * opp)
        over = first if depth_over_first else open_ & fin[p]
        counts[:, 2 * p], counts[:, 2 * p + 1], counts[:, 4 + p] = opp, same, fill
        counts[:, 6 + p] = np.where(over, d[p], 0).max((1, 2))
        shown = fin[p] & (open_ | heads[p] | (heads[q] if through_head else False))
        if head_minus_one:
            shown = shown & ~heads[p]
        dist[:, p] = np.where(shown, d[p], -1)
    counts[~playable[:, 0, 0]] = -1
    return counts, dist


WRONG_MODELS = {
    "absolute colour instead of the head's": dict(absolute_colour=True),
    "opp and same swapped in the fill formula": dict(swapped_fill=True),
    "2 min + 1 always": dict(always_plus_one=True),
    "first is everything reached": dict(reach_as_first=True),
    "the head's own cell is -1 in its plane": dict(head_minus_one=True),
    "the flood passes through the other head's cell": dict(through_head=True),
    "distances saturate at 255": dict(saturate=255),
    "distances saturate at 127": dict(saturate=127),
    "depth over first, not over the reached cells": dict(depth_over_first=True),
}


def winner(counts):
    """fill_winner: -2 for a rejected row, else 1 / 2 / 0 for fill1 greater than, less than, equal to fill2."""
    counts = np.asarray(counts)
    v = np.where(counts[:, FILL1] > counts[:, FILL2], 1, np.where(counts[:, FILL1] < counts[:, FILL2], 2, 0))
    return np.where(counts[:, FILL1] < 0, -2, v).astype(np.int8)


def owner_from_dist(dist, codes):
    """territory's owner plane from the two distance planes alone: 1 / 2 / 3 on the OPEN cells player 1 / player 2 / both
    at the same level come to first.  (A head's own 0 is no open cell.)"""
    d = np.where(dist < 0, np.int32(terr.INF), dist.astype(np.int32))
    cell = np.asarray(codes) == 1
    d1, d2 = d[:, 0], d[:, 1]
    return (cell * ((d1 < d2) * 1 + (d2 < d1) * 2 + ((d1 == d2) & (d1 < terr.INF)) * 3)).astype(np.int8)


# ---- the literal search: one board, a queue of cells, the header's sentences one by one ---------------------------------
def literal(board):
    """(counts list of 8, dist int16 [2, S, S]) of ONE board by a queue BFS per player."""
    board = np.asarray(board, np.int8)
    S = board.shape[0]
    dist = np.full((2, S, S), -1, np.int16)
    heads = []
    for byte in (10, -10):
        cells = [(r, c) for r in range(S) for c in range(S) if board[r, c] == byte]
        if len(cells) != 1 or not (1 <= cells[0][0] <= S - 2 and 1 <= cells[0][1] <= S - 2):
            return [-1] * 8, dist
        heads.append(cells[0])
    reached = []
    for p, head in enumerate(heads):
        d = {}
        queue, at = [(head, 0)], 0
        dist[p][head] = 0
        while at < len(queue):
            (r, c), l = queue[at]
            at += 1
            for cell in ((r - 1, c), (r, c + 1), (r + 1, c), (r, c - 1)):
                inside = 1 <= cell[0] <= S - 2 and 1 <= cell[1] <= S - 2
                if inside and board[cell] == 1 and cell not in d:
                    d[cell] = l + 1
                    dist[p][cell] = l + 1
                    queue.append((cell, l + 1))
        reached.append(d)
    counts = [0] * 8
    for p, head in enumerate(heads):
        mine, other = reached[p], reached[1 - p]
        opp = same = 0
        for cell, l in mine.items():
            if cell not in other or l < other[cell]:
                if (cell[0] + cell[1]) & 1 == (head[0] + head[1]) & 1:
                    same += 1
                else:
                    opp += 1
        counts[2 * p], counts[2 * p + 1] = opp, same
        counts[4 + p] = 2 * same + 1 if opp > same else 2 * opp
        counts[6 + p] = max(mine.values()) if mine else 0
    return counts, dist


def first_cells(board, p):
    """The set of first_p cells of one playable board and head p's cell, from the literal search."""
    _, dist = literal(board)
    S = board.shape[0]
    mine, other = dist[p], dist[1 - p]
    cells = {(r, c) for r in range(S) for c in range(S)
             if board[r, c] == 1 and mine[r, c] > 0 and (other[r, c] < 0 or mine[r, c] < other[r, c])}
    return cells, tuple(np.argwhere(board == (10, -10)[p])[0])


def longest_walk(cells, head):
    """The most moves a player at `head` can make inside `cells`, every cell once: exhaustive depth-first search."""
    best = 0

    def go(at, left, length):
        nonlocal best
        best = max(best, length)
        if best == len(cells):
            return
        r, c = at
        for nxt in ((r - 1, c), (r, c + 1), (r + 1, c), (r, c - 1)):
            if nxt in left:
                go(nxt, left - {nxt}, length + 1)

    go(head, frozenset(cells), 0)
    return best


# ---- the inputs ----------------------------------------------------------------------------------------------------------
def hand_boards(S):
    """Boards of one side, as tests/test_gpu_territory.py draws them: arenas with the heads in corners and side by side, an
    arena split by a wall row with and without a door (index 5 and 6: the last interior column is mask bit S - 2), the
    serpentine and its transpose, all of them again with a ring of ones, and two rejected boards."""
    out = [terr.arena(S, (1, 1), (S - 2, S - 2)), terr.arena(S, (S - 2, S - 2), (1, 1)), terr.arena(S, (1, S - 2), (S - 2, 1)),
           terr.arena(S, (S // 2, S // 2 - 1), (S // 2, S // 2)), terr.arena(S, (1, S - 2), (2, S - 2))]
    split = terr.arena(S, (1, S - 2), (S - 2, S - 2))
    split[S // 2, 1:-1] = -2
    door = split.copy()
    door[S // 2, S - 2] = 1
    out += [split, door, terr.serpentine(S), terr.serpentine(S).T.copy()]
    out += [terr.ring_of_ones(b) for b in list(out)]
    no_head, on_border = out[0].copy(), out[0].copy()
    no_head[1, 1] = 1
    on_border[1, 1], on_border[0, 1] = 1, 10
    return np.stack(out + [no_head, on_border])


def planted_boards(W):
    """What territory's boards do not hold, two boards: the serpentine and its transpose.  Its 297 levels at side 26 and
    525 at side 34 are what tells the two saturating models from the right one; below width 12 no board has 128 levels
    (W * W cells at most) and those two models are the right one."""
    S = W + 2
    return np.stack([terr.serpentine(S), terr.serpentine(S).T.copy()])


def can_differ(name, W):
    """Whether the wrong model `name` can depart from the model at width W at all: a saturating one needs a level above its limit."""
    return WRONG_MODELS[name].get("saturate", 0) < W * W


@ps.once
def boards(W):
    """Every board of width W the tests use: territory's (soup, early, planted), then the two planted here."""
    return np.concatenate([terr.boards(W), planted_boards(W)])


@ps.once
def expected(W):
    """model(boards(W))."""
    return model(boards(W))
