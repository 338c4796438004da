"""What the territory tests share (tests/test_territory_model_cpu.py, tests/test_gpu_territory.py): a vectorised numpy model
of tron_territory_codes as include/tron_hip.h defines it, a literal one-board queue BFS written independently of it, board
builders, the boards both files use, and a list of wrong models that the inputs must tell from the right one.  A plain
module, imported by name; nothing here needs a GPU."""
import numpy as np

import playout_support as ps

INF = np.int32(1 << 30)
FIRST1, FIRST2, TIED, NEITHER, REACH1, REACH2 = range(6)


# ---- the model -----------------------------------------------------------------------------------------------------------
def _flood(passable, start):
    """Breadth-first distances [n, S, S] from the True cells of `start` over `passable`, level by level; INF where the
    flood does not come.  The start cells themselves get 0."""
    n = len(passable)
    dist = np.full(passable.shape, INF, np.int32)
    dist[start] = 0
    rows = np.nonzero(start.any((1, 2)))[0]
    front, seen, ok = start[rows], start[rows].copy(), passable[rows]
    level = 0
    while len(rows):
        level += 1
        e = np.zeros_like(front)
        e[:, 1:, :] |= front[:, :-1, :]
        e[:, :-1, :] |= front[:, 1:, :]
        e[:, :, 1:] |= front[:, :, :-1]
        e[:, :, :-1] |= front[:, :, 1:]
        new = e & ok & ~seen
        sub = dist[rows]
        sub[new] = level
        dist[rows] = sub
        seen |= new
        keep = new.any((1, 2))
        rows, front, seen, ok = rows[keep], new[keep], seen[keep], ok[keep]
    return dist


def model(codes, ties_to_p1=False, through_head=False, open_border=False, neither_as_tied=False, reach_as_first=False,
          judge_rejected=False):
    """(counts int32 [n, 6], owner int8 [n, S, S]) of a stack of player-1 code boards.  The keywords are the WRONG models."""
    codes = np.ascontiguousarray(codes, np.int8)
    n, S = codes.shape[0], codes.shape[-1]
    inner = np.zeros((S, S), bool)
    inner[1:-1, 1:-1] = True
    open_ = codes == 1
    if not open_border:
        open_ = open_ & inner
    heads, playable = [], np.ones(n, bool)
    for byte in (10, -10):
        h = codes == byte
        playable &= (h.sum((1, 2)) == 1) & ((h & inner).sum((1, 2)) == 1)
        if judge_rejected:                                             # the first such byte, wherever it is
            first = np.zeros_like(h).reshape(n, -1)
            has = h.reshape(n, -1).any(1)
            first[np.nonzero(has)[0], h.reshape(n, -1).argmax(1)[has]] = True
            h = first.reshape(h.shape)
        heads.append(h)
    judged = np.ones(n, bool) if judge_rejected else playable
    d = []
    for p in range(2):
        passable = open_ | heads[1 - p] if through_head else open_
        dp = _flood(passable & judged[:, None, None], heads[p] & judged[:, None, None])
        d.append(np.where(open_, dp, INF))
    d1, d2 = d
    cell = open_ & judged[:, None, None]
    first1, first2 = cell & (d1 < d2), cell & (d2 < d1)
    tied, neither = cell & (d1 == d2) & (d1 < INF), cell & (d1 == INF) & (d2 == INF)
    if ties_to_p1:
        first1, tied = first1 | tied, np.zeros_like(tied)
    if neither_as_tied:
        tied, neither = tied | neither, np.zeros_like(neither)
    reach1, reach2 = cell & (d1 < INF), cell & (d2 < INF)
    if reach_as_first:
        reach1, reach2 = first1 | tied, first2 | tied
    counts = np.stack([m.sum((1, 2)) for m in (first1, first2, tied, neither, reach1, reach2)], 1).astype(np.int32)
    owner = (first1 * 1 + first2 * 2 + tied * 3).astype(np.int8)
    counts[~judged] = -1
    owner[~judged] = 0
    return counts, owner


WRONG_MODELS = {
    "ties go to player 1": dict(ties_to_p1=True),
    "the flood passes through the other head's cell": dict(through_head=True),
    "the border ring is open where its byte is 1": dict(open_border=True),
    "neither is counted as tied": dict(neither_as_tied=True),
    "reach is first + tied": dict(reach_as_first=True),
    "a rejected board is judged as if playable": dict(judge_rejected=True),
}


def winner(counts):
    """territory_winner: -2 for a rejected row, else 1 / 2 / 0 for first1 greater than, less than, equal to first2."""
    counts = np.asarray(counts)
    v = np.where(counts[:, 0] > counts[:, 1], 1, np.where(counts[:, 0] < counts[:, 1], 2, 0))
    return np.where(counts[:, 0] < 0, -2, v).astype(np.int8)


# ---- the literal search: one board, a queue of cells, the header's sentences one by one ---------------------------------
def literal(board):
    """(counts list of 6, owner int8 [S, S]) of ONE board by a queue BFS per player."""
    board = np.asarray(board, np.int8)
    S = board.shape[0]
    where = {10: [], -10: []}
    for r in range(S):
        for c in range(S):
            if int(board[r, c]) in where:
                where[int(board[r, c])].append((r, c))
    owner = np.zeros((S, S), np.int8)
    for cells in where.values():
        if len(cells) != 1 or not (1 <= cells[0][0] <= S - 2 and 1 <= cells[0][1] <= S - 2):
            return [-1] * 6, owner

    def is_open(r, c):
        return 1 <= r <= S - 2 and 1 <= c <= S - 2 and board[r, c] == 1

    dist = []
    for byte in (10, -10):
        d = {}
        queue, at = [(where[byte][0], 0)], 0                          # a list read from the front
        while at < len(queue):
            (r, c), l = queue[at]
            at += 1
            for rr, cc in ((r - 1, c), (r, c + 1), (r + 1, c), (r, c - 1)):
                if is_open(rr, cc) and (rr, cc) not in d:
                    d[(rr, cc)] = l + 1
                    queue.append(((rr, cc), l + 1))
        dist.append(d)
    counts = [0] * 6
    for r in range(S):
        for c in range(S):
            if not is_open(r, c):
                continue
            a, b = dist[0].get((r, c)), dist[1].get((r, c))
            if a is not None:
                counts[REACH1] += 1
            if b is not None:
                counts[REACH2] += 1
            if a is None and b is None:
                counts[NEITHER] += 1
            elif b is None or (a is not None and a < b):
                counts[FIRST1] += 1
                owner[r, c] = 1
            elif a is None or b < a:
                counts[FIRST2] += 1
                owner[r, c] = 2
            else:
                counts[TIED] += 1
                owner[r, c] = 3
    return counts, owner


# ---- board builders ------------------------------------------------------------------------------------------------------
_BYTE = {"#": -1, ".": 1, "A": 10, "B": -10, "a": -2, "b": -3}


def draw(rows):
    """A board from text: '#' wall, '.' empty, 'A' / 'B' the +10 / -10 head, 'a' / 'b' their bodies."""
    rows = [r.replace(" ", "") for r in rows]
    assert all(len(r) == len(rows) for r in rows), rows
    return np.array([[_BYTE[ch] for ch in r] for r in rows], np.int8)


def arena(S, h1, h2):
    """An empty S x S arena with a wall ring and the heads at (row, column) h1 and h2."""
    b = np.full((S, S), -1, np.int8)
    b[1:-1, 1:-1] = 1
    b[h1], b[h2] = 10, -10
    return b


def serpentine(S):
    """One long corridor through an S x S arena: every other interior row is a wall with a door at alternating ends.  The
    +10 head sits at the corridor's start, the -10 head in a sealed cell in the last row, so player 1 floods the whole
    corridor alone, hundreds of levels deep at side 34."""
    walls = list(range(2, S - 2, 2))
    last_door = S - 2 if len(walls) % 2 == 1 else 1
    col, step = (1, 1) if last_door == S - 2 else (S - 2, -1)          # player 2: the last row's corner away from the door
    b = arena(S, (1, 1), (S - 2, col))
    for k, r in enumerate(walls):
        b[r, 1:-1] = -2
        b[r, S - 2 if k % 2 == 0 else 1] = 1
    b[S - 2, col + step] = b[S - 3, col] = -3                          # the sealed cell of player 2
    return b


def ring_of_ones(boards):
    """The same boards with every byte of the border ring set to 1."""
    out = np.array(boards, np.int8, copy=True)
    out[..., 0, :] = out[..., -1, :] = 1
    out[..., :, 0] = out[..., :, -1] = 1
    return out


# ---- the inputs ----------------------------------------------------------------------------------------------------------
WIDTHS = ps.SOUP_WIDTHS                                                # 4, 5, 10, 24, 32: sides 6, 7, 12, 26, 34
EARLY_N = 512
PLANT_N = 320


def early_boards(W, n=EARLY_N, seed=None):
    """The soup's recipe (playout_support.soup_boards) with at most W steps played, rejected boards included."""
    rs = np.random.RandomState(7000 + W if seed is None else seed)
    return ps.spoil_some(ps.stopped_games(rs, W, n, W + 1, stream_id=4))


def planted_boards(W, n=PLANT_N):
    """Boards the soups hardly ever hold, n of each kind, as round 27 planted dead ends:
      doors     a wall across the arena with one door, the -10 head IN the door and the +10 head on one side: everything
                behind the door is reached by player 1 only if the flood passes through the other head;
      pockets   the same wall without a door and both heads on one side: the other side is reached by neither;
      rings     early boards whose border ring holds 1 in a random half of its bytes (or in all of them);
      rejected  early boards with a head removed, doubled or moved onto the border, for either player."""
    rs = np.random.RandomState(9000 + W)
    S = W + 2
    doors, pockets = [], []
    for k in range(2 * n):
        b = np.full((S, S), -1, np.int8)
        b[1:-1, 1:-1] = np.where(rs.rand(W, W) < 0.06, -2 - (k & 1), 1)
        across = bool(rs.randint(2)) and W > 2
        line = rs.randint(2, S - 2)                                    # interior line 2..S-3: cells on both sides
        v = b.T if across else b
        v[line, 1:-1] = -3 + (k & 1)
        side = -1 if rs.randint(2) else 1
        if k < n:
            door = rs.randint(1, S - 1)
            v[line, door] = -10
            v[line - side, door] = 1                                   # the cell player 1 would enter behind the door
            free = [(line + side, c) for c in range(1, S - 1)]
            v[free[rs.randint(len(free))]] = 10
            doors.append(b)
        else:
            rows = [r for r in range(1, S - 1) if (r - line) * side > 0]
            cells = [(r, c) for r in rows for c in range(1, S - 1)]
            i, j = rs.choice(len(cells), 2, replace=False)
            v[cells[i]], v[cells[j]] = 10, -10
            pockets.append(b)
    base = early_boards(W, 2 * n, seed=9100 + W)
    for i in range(2 * n):                                             # playable bases only
        if (base[i] == 10).sum() != 1 or not (base[i][1:-1, 1:-1] == 10).any():
            base[i] = arena(S, (1, 1), (S - 2, S - 2))
    rings = base[:n].copy()
    ring = np.ones((S, S), bool)
    ring[1:-1, 1:-1] = False
    for i in range(n):
        on = ring & ((rs.rand(S, S) < 0.5) | (i % 3 == 0))
        rings[i][on] = 1
    rejected = base[n:].copy()
    for i in range(n):
        b, byte = rejected[i], (10, -10)[i & 1]
        r, c = np.argwhere(b == byte)[0]
        kind = (i >> 1) % 3
        if kind == 0:                                                  # no such head
            b[r, c] = -2
        elif kind == 1:                                                # two of them
            e = np.argwhere(b == 1)
            if len(e):
                b[tuple(e[rs.randint(len(e))])] = byte
            else:
                b[0, 0] = byte
        else:                                                          # on the border
            b[r, c] = -2
            b[(0, c) if rs.randint(2) else (r, S - 1)] = byte
    return np.concatenate([np.stack(doors), np.stack(pockets), rings, rejected])


@ps.once
def boards(W):
    """Every board of width W the tests use: the soup, the early boards, the planted boards."""
    return np.concatenate([ps.soup_boards(W), early_boards(W), planted_boards(W)])


@ps.once
def expected(W):
    """model(boards(W))."""
    return model(boards(W))
