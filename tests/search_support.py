"""What the search tests share (tests/test_search_model_cpu.py, tests/test_gpu_search.py): a vectorised numpy model of
tron_search_codes as include/tron_hip.h defines it, built on territory_support's flood and model and flooding only the lines
that are live somewhere; a literal one-board recursive search with a queue BFS of its own, written sentence by sentence from
the header and sharing no code with the model; the wrong models that the inputs must tell from the right one; the planted
positions and the boards (reach_support's, with the planted ones behind them).  A plain module, imported by name; nothing
here needs a GPU."""
import numpy as np

import playout_support as ps
import reach_support as rch
import territory_support as terr

DELTAS = ((-1, 0), (0, 1), (1, 0), (0, -1))                            # UP, RIGHT, DOWN, LEFT: (row, column)
DECIDED = 2048
REJECTED = -2 ** 31
NOT_PLAYED = -(1 << 30)                                                # what one wrong model leaves in an unsafe move's slot
PLIES = (1, 2, 3)


# ---- the model -----------------------------------------------------------------------------------------------------------
def _leaf(open_, h1, h2, reach=False):
    """first1 - first2 (int64 [m]) of the positions (open_, h1, h2), all of them live: both floods in one call."""
    m = len(open_)
    d = terr._flood(np.concatenate([open_, open_]), np.concatenate([h1, h2]))
    d1, d2 = np.where(open_, d[:m], terr.INF), np.where(open_, d[m:], terr.INF)
    if reach:
        return (d1 < terr.INF).sum((1, 2)).astype(np.int64) - (d2 < terr.INF).sum((1, 2))
    return (d1 < d2).sum((1, 2)).astype(np.int64) - (d2 < d1).sum((1, 2))


def _node(open_, h1, h2, k, r, w):
    """(U_1 int64 [m, 4], U_2 int64 [m, 4]) of the m positions (open_, h1, h2) reached after k joint moves, r plies left."""
    m = len(open_)
    t1 = [np.roll(h1, d, (1, 2)) for d in DELTAS]                      # a head is strictly inside: nothing wraps
    t2 = [np.roll(h2, d, (1, 2)) for d in DELTAS]
    s1 = np.stack([(t & open_).any((1, 2)) for t in t1], 1)
    s2 = np.stack([(t & open_).any((1, 2)) for t in t2], 1)
    term = DECIDED if w["no_minus_k"] else DECIDED + k if w["plus_k"] else DECIDED - k
    fold = np.maximum if w["max_over_b"] else np.minimum
    start = -(1 << 40) if w["max_over_b"] else 1 << 40
    u1, u2 = np.full((m, 4), start, np.int64), np.full((m, 4), start, np.int64)
    for a in range(4):
        for b in range(4):
            same = (t1[a] & t2[b]).any((1, 2)) & s1[:, a] & s2[:, b]
            draw = (~s1[:, a] & ~s2[:, b]) | same
            w1 = np.where(draw, 0, np.where(s1[:, a], term, -term)).astype(np.int64)
            w2 = -w1
            if w["draw_as_loss"]:
                w1, w2 = np.where(draw, -term, w1), np.where(draw, -term, w2)
            if w["collision_to_p1"]:
                w1, w2 = np.where(same, term, w1), np.where(same, -term, w2)
            on = np.nonzero(s1[:, a] & s2[:, b] & ~same)[0]
            if len(on):                                                # only the boards that have this line go down it
                child = open_[on] & ~t1[a][on] & ~t2[b][on]
                if w["reopen_head"]:
                    child = child | h1[on] | h2[on]
                if r == 1:
                    if w["leaf_on_parent"]:
                        v1 = _leaf(open_[on], h1[on], h2[on])
                    else:
                        v1 = _leaf(child, t1[a][on], t2[b][on], reach=w["leaf_reach"])
                    v2 = -v1
                else:
                    c1, c2 = _node(child, t1[a][on], t2[b][on], k + 1, r - 1, w)
                    v1, v2 = c1.max(1), c2.max(1)
                    if w["v2_neg_v1"]:
                        v2 = -v1
                w1[on], w2[on] = v1, v2
            u1[:, a] = fold(u1[:, a], w1)
            u2[:, b] = fold(u2[:, b], w2)
    if w["unsafe_skipped"]:
        u1[~s1], u2[~s2] = NOT_PLAYED, NOT_PLAYED
    return u1, u2


_WRONG = ("draw_as_loss", "collision_to_p1", "no_minus_k", "plus_k", "v2_neg_v1", "max_over_b", "leaf_reach",
          "leaf_on_parent", "reopen_head", "last_tie", "unsafe_skipped")


def model(codes, plies, **wrong):
    """(values int32 [n, 2, 4], actions int8 [n, 2]) of a stack of player-1 code boards.  The keywords (_WRONG) are the
    WRONG models."""
    w = dict.fromkeys(_WRONG, False)
    assert set(wrong) <= set(w) and plies in PLIES
    w.update(wrong)
    codes = np.ascontiguousarray(codes, np.int8)
    n, S = codes.shape[0], codes.shape[-1]
    inner = np.zeros((S, S), bool)
    inner[1:-1, 1:-1] = True
    playable = terr.model(codes)[0][:, 0] >= 0
    values = np.full((n, 2, 4), REJECTED, np.int64)
    actions = np.full((n, 2), -1, np.int8)
    at = np.nonzero(playable)[0]
    if len(at):
        c = codes[at]
        u1, u2 = _node((c == 1) & inner, c == 10, c == -10, 0, plies, w)
        u = np.stack([u1, u2], 1)
        values[at] = u
        actions[at] = (3 - u[..., ::-1].argmax(-1)) if w["last_tie"] else u.argmax(-1)
    return values.astype(np.int32), actions


WRONG_MODELS = {
    "a draw scored as a loss for both": dict(draw_as_loss=True),
    "a same-cell collision given to player 1": dict(collision_to_p1=True),
    "terminal values without the - k": dict(no_minus_k=True),
    "terminal values with + k": dict(plus_k=True),
    "V_2 taken as -V_1": dict(v2_neg_v1=True),
    "max over b (optimistic)": dict(max_over_b=True),
    "the leaf is reach1 - reach2": dict(leaf_reach=True),
    "the leaf on the parent position": dict(leaf_on_parent=True),
    "the vacated head cell reopened": dict(reopen_head=True),
    "the last instead of the first direction on ties": dict(last_tie=True),
    "an unsafe own move valued as not played": dict(unsafe_skipped=True),
}


def can_differ(name, plies):
    """Whether the wrong model `name` can depart from the model at this depth at all: a terminal's k is 0 at the root, and
    V_2 = -V_1 holds at a leaf."""
    return plies > 1 or name not in ("terminal values without the - k", "terminal values with + k", "V_2 taken as -V_1")


def drawn_replies(codes):
    """bool [n, 2, 4]: whether player p's root move a has a reply that draws the first joint move (both unsafe, or both safe
    onto one cell), from the safety bits of the position alone.  All False on a rejected board."""
    codes = np.ascontiguousarray(codes, np.int8)
    S = codes.shape[-1]
    inner = np.zeros((S, S), bool)
    inner[1:-1, 1:-1] = True
    playable = (terr.model(codes)[0][:, 0] >= 0)[:, None, None]
    open_ = (codes == 1) & inner & playable
    t = [[np.roll((codes == byte) & playable, d, (1, 2)) for d in DELTAS] for byte in (10, -10)]
    s = [np.stack([(x & open_).any((1, 2)) for x in t[p]], 1) for p in (0, 1)]
    draw = np.stack([np.stack([(~s[0][:, a] & ~s[1][:, b] & playable[:, 0, 0]) | ((t[0][a] & t[1][b]).any((1, 2)) & s[0][:, a])
                               for b in range(4)], 1) for a in range(4)], 1)            # [n, a, b]
    return np.stack([draw.any(2), draw.any(1)], 1)


def kinds(values, codes):
    """What the root values of `codes` are: bool arrays (win, loss, territory, draw).  A decided line is worth at least
    2048 - 2 either way and a nonzero value below that is a territory difference, from the number alone; a draw is a zero
    on a move that has a drawn reply at the root (the minimum is then the draw's, or ties with it)."""
    v = np.asarray(values).astype(np.int64)
    return (v >= DECIDED - 2, (v <= 2 - DECIDED) & (v > REJECTED), (v != 0) & (abs(v) < DECIDED - 2),
            (v == 0) & drawn_replies(codes))


# ---- the literal search: one board, recursion over the joint moves, a queue of cells -----------------------------------
def literal(board, plies):
    """(values: 2 lists of 4, actions: list of 2) of ONE board, sentence by sentence from the header."""
    board = np.asarray(board, np.int8)
    S = board.shape[0]
    heads = []
    for byte in (10, -10):
        cells = [(r, c) for r in range(S) for c in range(S) if board[r, c] == byte]
        if len(cells) != 1 or not (1 <= cells[0][0] <= S - 2 and 1 <= cells[0][1] <= S - 2):
            return [[REJECTED] * 4, [REJECTED] * 4], [-1, -1]
        heads.append(cells[0])
    O = frozenset((r, c) for r in range(1, S - 1) for c in range(1, S - 1) if board[r, c] == 1)

    def distances(O, head):
        d, queue, at = {}, [(head, 0)], 0
        while at < len(queue):
            (r, c), l = queue[at]
            at += 1
            for dr, dc in DELTAS:
                cell = (r + dr, c + dc)
                if cell in O and cell not in d:
                    d[cell] = l + 1
                    queue.append((cell, l + 1))
        return d

    def V(O, h, p, k, r):
        if r == 0:
            d = [distances(O, h[0]), distances(O, h[1])]
            first = [sum(1 for cell in O if cell in d[x] and (cell not in d[1 - x] or d[x][cell] < d[1 - x][cell])) for x in (0, 1)]
            return first[p] - first[1 - p]
        return max(U(O, h, p, k, r))

    def U(O, h, p, k, r):
        q = 1 - p
        out = []
        for a in range(4):
            worst = None
            for b in range(4):
                mine = (h[p][0] + DELTAS[a][0], h[p][1] + DELTAS[a][1])
                theirs = (h[q][0] + DELTAS[b][0], h[q][1] + DELTAS[b][1])
                safe_p, safe_q = mine in O, theirs in O
                if (not safe_p and not safe_q) or (safe_p and safe_q and mine == theirs):
                    w = 0
                elif not safe_q:
                    w = DECIDED - k
                elif not safe_p:
                    w = -(DECIDED - k)
                else:
                    new = [None, None]
                    new[p], new[q] = mine, theirs
                    w = V(O - {mine, theirs}, new, p, k + 1, r - 1)
                worst = w if worst is None or w < worst else worst
            out.append(worst)
        return out

    values = [U(O, heads, p, 0, plies) for p in (0, 1)]
    return values, [v.index(max(v)) for v in values]


# ---- the inputs ----------------------------------------------------------------------------------------------------------
PLANTED = {
    "two apart": ["#######", "#.....#", "#.....#", "#.A.B.#", "#.....#", "#.....#", "#######"],
    "adjacent": ["#######", "#.....#", "#.....#", "#..AB.#", "#.....#", "#.....#", "#######"],
    "dead end": ["#######", "#a###.#", "#A..#.#", "#####.#", "#....B#", "#.....#", "#######"],
    "boxed in": ["#######", "#A#.#B#", "###.###", "#.....#", "#.....#", "#.....#", "#######"],
    "lopsided": ["#######", "#A...##", "#.##.##", "#....B#", "#.##..#", "#....##", "#######"],
}
PLANTED_NAMES = tuple(PLANTED)


def planted(S):
    """The planted 7 x 7 positions in the top-left corner of a walled S x S image, in PLANTED's order, then each of them
    with the two players' bytes exchanged."""
    out = []
    for rows in PLANTED.values():
        b = np.full((S, S), -1, np.int8)
        b[:7, :7] = terr.draw(rows)
        out.append(b)
    swapped = []
    for b in out:
        s = b.copy()
        s[b == 10], s[b == -10], s[b == -2], s[b == -3] = -10, 10, -3, -2
        swapped.append(s)
    return np.stack(out + swapped)


@ps.once
def boards(W):
    """Every board of width W the tests use: reach_support's (territory's soup, early and planted boards, the serpentines),
    then the positions planted here (width 5 and up)."""
    return np.concatenate([rch.boards(W), planted(W + 2)]) if W >= 5 else rch.boards(W)


# plies 3 runs on slices: a few hundred boards at the small widths, a few dozen at the large ones, the planted ones last
def deep_boards(W):
    b = boards(W)
    if W <= 10:
        return np.concatenate([b[:96], b[1061:1125], b[1573:1637], b[-76:]])
    return np.concatenate([b[:12], b[1061:1067], b[-14:]])


@ps.once
def expected(W, plies):
    """model(...): boards(W) at plies 1 and 2, deep_boards(W) at plies 3."""
    return model(deep_boards(W) if plies == 3 else boards(W), plies)
