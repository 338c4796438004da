"""What the moves tests share (tests/test_moves_model_cpu.py, tests/test_gpu_moves.py): a vectorised numpy model of
tron_moves_codes as include/tron_hip.h defines it, built on territory_support's flood; a literal one-board queue BFS written
independently of it, sentence by sentence from the header; the wrong models that the inputs must tell from the right one;
the boards (reach_support's).  A plain module, imported by name; nothing here needs a GPU."""
import numpy as np

import playout_support as ps
import reach_support as rch
import territory_support as terr

ROOM, FILL, FIRST = range(3)
DELTAS = ((-1, 0), (0, 1), (1, 0), (0, -1))                            # UP, RIGHT, DOWN, LEFT: (row, column)


# ---- the model -----------------------------------------------------------------------------------------------------------
def _pick(keys, safe):
    """The first safe direction of the greatest key (int64 [n, 2, 4], any value on an unsafe move), 0 when none is safe."""
    return np.where(safe, keys, -1).argmax(-1).astype(np.int8)


def floods(codes, through_own_head=False, through_other_head=False, open_border=False):
    """What every model of one stack shares, the eight target floods and the two head floods: a dict of playable [n],
    open [n, S, S], heads (two [n, S, S]), d int32 [n, 2, S, S] (INF off the open cells), target bool and e int32
    [n, 2, 4, S, S].  The keywords are WRONG models of the floods."""
    codes = np.ascontiguousarray(codes, np.int8)
    n, S = codes.shape[0], codes.shape[-1]
    inner = np.zeros((S, S), bool)
    inner[1:-1, 1:-1] = True
    playable = terr.model(codes)[0][:, 0] >= 0
    open_ = (codes == 1) & playable[:, None, None]
    if not open_border:
        open_ = open_ & inner
    heads = [(codes == 10) & playable[:, None, None], (codes == -10) & playable[:, None, None]]
    d = np.stack([np.where(open_, terr._flood(open_, heads[p]), terr.INF) for p in range(2)], 1)
    target = np.zeros((n, 2, 4, S, S), bool)
    e = np.zeros((n, 2, 4, S, S), np.int32)
    for p in range(2):
        passable = open_
        if through_own_head:
            passable = passable | heads[p]
        if through_other_head:
            passable = passable | heads[1 - p]
        for a, (dr, dc) in enumerate(DELTAS):
            target[:, p, a] = np.roll(heads[p], (dr, dc), (1, 2)) & open_          # a head is strictly inside: nothing wraps
            e[:, p, a] = terr._flood(passable, target[:, p, a])
    return dict(playable=playable, open=open_, heads=heads, d=d, target=target, e=e)


def model(codes, pick="first_fill", first_le=False, first_no_plus_one=False, room_without_t=False, head_colour=False,
          unsafe_zero=False, given=None, details=False, **flood_kw):
    """(moves int32 [n, 2, 4, 3], actions int8 [n, 2]) of a stack of player-1 code boards.  The keywords, floods' among
    them, are the WRONG models.  given: floods(codes) made earlier.  details=True adds that dict, with `reached` bool
    [n, 2, 4, S, S] in it."""
    fl = dict(floods(codes, **flood_kw) if given is None else given)
    playable, open_, heads, d = fl["playable"], fl["open"], fl["heads"], fl["d"]
    n, S = open_.shape[0], open_.shape[-1]
    colour = (np.add.outer(np.arange(S), np.arange(S)) & 1)[None]
    moves = np.zeros((n, 2, 4, 3), np.int64)
    safe = fl["target"].any((3, 4))
    reached = np.zeros((n, 2, 4, S, S), bool)
    for p in range(2):
        dq = d[:, 1 - p]
        for a in range(4):
            t, e = fl["target"][:, p, a], fl["e"][:, p, a]
            fin = (e < terr.INF) & open_
            ref = (colour * (heads[p] if head_colour else t)).sum((1, 2))[:, None, None]
            same = (fin & (colour == ref)).sum((1, 2))
            opp = fin.sum((1, 2)) - same
            mine = e if first_no_plus_one else e + 1
            ahead = (mine <= dq) if first_le else (mine < dq)
            moves[:, p, a, ROOM] = fin.sum((1, 2)) - (safe[:, p, a] if room_without_t else 0)
            moves[:, p, a, FILL] = np.where(same > opp, 2 * opp + 1, 2 * same)
            moves[:, p, a, FIRST] = (fin & ((dq >= terr.INF) | ahead)).sum((1, 2))
            reached[:, p, a] = fin
    keys = {"first_fill": moves[..., FIRST] * 4096 + moves[..., FILL], "first": moves[..., FIRST],
            "fill_first": moves[..., FILL] * 4096 + moves[..., FIRST], "room": moves[..., ROOM]}[pick]
    actions = _pick(keys, safe)
    moves[~safe] = 0 if unsafe_zero else -1
    moves[~playable] = -1
    actions[~playable] = -1
    fl["reached"] = reached
    out = moves.astype(np.int32), actions
    return out + (fl,) if details else out


WRONG_MODELS = {
    "the pick by first alone": dict(pick="first"),
    "the pick by (fill, first)": dict(pick="fill_first"),
    "the pick by room": dict(pick="room"),
    "first with <= instead of <": dict(first_le=True),
    "first without the + 1": dict(first_no_plus_one=True),
    "room without t": dict(room_without_t=True),
    "colour taken from the head instead of from t": dict(head_colour=True),
    "the flood passes through the own head's cell": dict(through_own_head=True),
    "the flood passes through the other head's cell": dict(through_other_head=True),
    "the border ring is open where its byte is 1": dict(open_border=True),
    "an unsafe move is zeros instead of -1": dict(unsafe_zero=True),
}


def safe(moves):
    """safe_moves: room >= 0."""
    return np.asarray(moves)[..., ROOM] >= 0


# ---- the literal search: one board, a queue of cells, the header's sentences one by one ---------------------------------
def literal(board):
    """(moves: 2 x 4 lists of [room, fill, first], actions: list of 2) of ONE board by queue BFS."""
    board = np.asarray(board, np.int8)
    S = board.shape[0]
    heads = []
    for byte in (10, -10):
        cells = [(r, c) for r in range(S) for c in range(S) if board[r, c] == byte]
        if len(cells) != 1 or not (1 <= cells[0][0] <= S - 2 and 1 <= cells[0][1] <= S - 2):
            return [[[-1, -1, -1] for _ in range(4)] for _ in range(2)], [-1, -1]
        heads.append(cells[0])

    def is_open(cell):
        return 1 <= cell[0] <= S - 2 and 1 <= cell[1] <= S - 2 and board[cell] == 1

    def bfs(queue, found):
        at = 0
        while at < len(queue):
            (r, c), l = queue[at]
            at += 1
            for dr, dc in DELTAS:
                cell = (r + dr, c + dc)
                if is_open(cell) and cell not in found:
                    found[cell] = l + 1
                    queue.append((cell, l + 1))
        return found

    d = [bfs([(head, 0)], {}) for head in heads]                       # d_p over open cells: a neighbour of the head has 1
    moves, actions = [], []
    for p, (hr, hc) in enumerate(heads):
        other = d[1 - p]
        rows, best = [], None
        for a, (dr, dc) in enumerate(DELTAS):
            t = (hr + dr, hc + dc)
            if not is_open(t):
                rows.append([-1, -1, -1])
                continue
            e = bfs([(t, 0)], {t: 0})
            same = sum(1 for (r, c) in e if (r + c) & 1 == (t[0] + t[1]) & 1)
            opp = len(e) - same
            fill = 2 * opp + 1 if same > opp else 2 * same
            first = sum(1 for cell, l in e.items() if cell not in other or 1 + l < other[cell])
            rows.append([len(e), fill, first])
            if best is None or (first, fill) > best[0]:
                best = ((first, fill), a)
        moves.append(rows)
        actions.append(0 if best is None else best[1])
    return moves, actions


# ---- the inputs ----------------------------------------------------------------------------------------------------------
@ps.once
def boards(W):
    """Every board of width W the tests use: reach_support's (territory's soup, early and planted boards, the serpentines)."""
    return rch.boards(W)


@ps.once
def expected(W):
    """model(boards(W))."""
    return model(boards(W))
