"""The host model of tron_territory_codes (tests/territory_support.py): it equals a literal queue BFS on every board the GPU
tests use, the header's identities hold, hand-drawn boards give the six numbers written here, the reference's Voronoi
leaf value rebuilt from the model equals oracle.minimax_move's root values, and the inputs tell every wrong model from the
right one on at least one board in ten at every width."""
import numpy as np
import pytest

import oracle
import playout_support as ps
import territory_support as terr


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_model_equals_literal_bfs(W):
    boards = terr.boards(W)
    counts, owner = terr.expected(W)
    for i, b in enumerate(boards):
        lc, lo = terr.literal(b)
        assert list(counts[i]) == lc, (W, i)
        assert np.array_equal(owner[i], lo), (W, i)


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_identities(W):
    boards = terr.boards(W)
    counts, owner = terr.expected(W)
    rejected = counts[:, 0] < 0
    assert rejected.any() and not rejected.all()
    assert (counts[rejected] == -1).all() and not owner[rejected].any()
    c, b, o = counts[~rejected].astype(np.int64), boards[~rejected], owner[~rejected]
    open_cells = (b[:, 1:-1, 1:-1] == 1).sum((1, 2))
    assert np.array_equal(c[:, 0] + c[:, 1] + c[:, 2] + c[:, 3], open_cells)
    both = c[:, 4] + c[:, 5] - (c[:, 0] + c[:, 1] + c[:, 2])
    assert (both >= 0).all()
    for k in (1, 2, 3):
        assert np.array_equal((o == k).sum((1, 2)), c[:, k - 1])
    assert not o[b != 1].any()
    # separated: no open cell next to cells of both floods <=> nothing is reached by both
    separated = both == 0
    assert separated.any() and not separated.all()
    assert (c[separated, 2] == 0).all()
    assert np.array_equal(c[separated, 4], c[separated, 0]) and np.array_equal(c[separated, 5], c[separated, 1])


HAND = {
    "an empty arena": (["######",
                        "#A...#",
                        "#....#",
                        "#....#",
                        "#...B#",
                        "######"], [5, 5, 4, 0, 14, 14]),
    "a wall between the players": (["#######",
                                    "#A.a..#",
                                    "#..a..#",
                                    "#..a.B#",
                                    "#..a..#",
                                    "#..a..#",
                                    "#######"], [9, 9, 0, 0, 9, 9]),
    "a one-cell door": (["#######",
                         "#A.a..#",
                         "#..a..#",
                         "#..a.B#",
                         "#..a..#",
                         "#.....#",
                         "#######"], [8, 10, 1, 0, 19, 19]),
    "a head boxed in": (["######",
                         "#Aa..#",
                         "#a...#",
                         "#....#",
                         "#...B#",
                         "######"], [0, 12, 0, 0, 0, 12]),
    "heads adjacent": (["######",
                        "#....#",
                        "#.AB.#",
                        "#....#",
                        "#....#",
                        "######"], [7, 7, 0, 0, 14, 14]),
    "a pocket neither reaches": (["#######",
                                  "#A.b..#",
                                  "#..b..#",
                                  "#B.bbb#",
                                  "#.....#",
                                  "#.....#",
                                  "#######"], [1, 11, 2, 4, 14, 14]),
}


@pytest.mark.parametrize("name", HAND)
def test_hand_drawn_boards(name):
    rows, want = HAND[name]
    board = terr.draw(rows)
    counts, owner = terr.model(board[None])
    lc, lo = terr.literal(board)
    assert list(counts[0]) == want and lc == want, (name, list(counts[0]), lc)
    assert np.array_equal(owner[0], lo)
    ring = terr.ring_of_ones(board)                                      # the ring's bytes change nothing
    rc, ro = terr.model(ring[None])
    assert list(rc[0]) == want and np.array_equal(ro[0], owner[0])


def test_serpentine_is_deep():
    board = terr.serpentine(34)
    counts, _ = terr.model(board[None])
    assert list(counts[0]) == terr.literal(board)[0]
    assert counts[0, 0] == counts[0, 4] > 500 and counts[0, 1] == counts[0, 5] == 0 and counts[0, 3] == 0


def test_winner():
    counts = np.array([[3, 2, 0, 0, 3, 2], [2, 3, 9, 0, 9, 9], [4, 4, 0, 1, 4, 4], [-1] * 6, [0, 0, 0, 0, 0, 0]], np.int32)
    assert list(terr.winner(counts)) == [1, 2, 0, -2, 0]


@pytest.mark.parametrize("W", (4, 5, 10))
def test_model_rebuilds_the_reference_voronoi_values(W, capsys):
    """tron_minimax.hip's header: a leaf's value is first_me - first_opp - neither + enemy-body cells, on the leaf map after
    my move a and the opponent's b (the two old heads closed, the new heads the flood's starts); a root child is the
    minimum over the opponent's unblocked moves, 0 when it has none.  Rebuilt from the model on the boards where no reply
    is a crash (the opponent stepping onto my new head changes the leaf's start cell) and compared with the oracle, which
    is pinned to the recorded reference searches."""
    boards = ps.soup_boards(W)
    _, pos, playable = ps.decode(boards)
    S = W + 2
    leaves, where, expect, covered = [], [], [], []
    for i in np.nonzero(playable)[0][::3]:
        b = boards[i]
        (r0, c0), (r1, c1) = (int(x) + 1 for x in pos[i, :2]), (int(x) + 1 for x in pos[i, 2:])
        mine = [(r0 + ps.DR[a], c0 + ps.DC[a]) for a in range(4)]
        theirs = [(r1 + ps.DR[a], c1 + ps.DC[a]) for a in range(4)]
        root_ok = [b[t] == 1 for t in mine]
        if any(ok and u == t for t, ok in zip(mine, root_ok) for u in theirs):
            continue                                                   # a crash reply
        covered.append(i)
        for a, t in enumerate(mine):
            for u in theirs:
                if root_ok[a] and b[u] == 1:
                    leaf = b.copy()
                    leaf[r0, c0], leaf[r1, c1] = -2, -2                # closed, and no enemy body (those are counted on b)
                    leaf[t], leaf[u] = 10, -10
                    leaves.append(leaf)
                    where.append((len(covered) - 1, a))
    counts, _ = terr.model(np.stack(leaves))
    assert (counts >= 0).all()
    values = np.zeros((len(covered), 4), np.int64)
    seen = np.zeros((len(covered), 4), bool)
    for (k, a), c in zip(where, counts.astype(np.int64)):
        v = c[0] - c[1] - c[3] + int((boards[covered[k]] == -3).sum())
        values[k, a] = min(values[k, a], v) if seen[k, a] else v
        seen[k, a] = True
    for k, i in enumerate(covered):
        _, ov, oe, _ = oracle.minimax_move(boards[i], 2, 0, np.zeros(8, np.uint32))
        b = boards[i]
        r0, c0 = (int(x) + 1 for x in pos[i, :2])
        assert [bool(b[r0 + ps.DR[a], c0 + ps.DC[a]] == 1) for a in range(4)] == list(oe), (W, i)
        assert list(ov) == list(values[k]), (W, i, list(ov), list(values[k]))
    with capsys.disabled():
        print(f"\n  W={W}: {len(covered)} boards without a crash reply of {len(np.nonzero(playable)[0][::3])} tried, "
              f"{len(leaves)} leaves, root values equal")
    assert len(covered) >= 100


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_inputs_tell_every_wrong_model(W, capsys):
    """A condition on the inputs: every wrong model departs from the model on at least one board in ten."""
    boards = terr.boards(W)
    counts, owner = terr.expected(W)
    shares = {}
    for name, kw in terr.WRONG_MODELS.items():
        wc, wo = terr.model(boards, **kw)
        shares[name] = float(((wc != counts).any(1) | (wo != owner).any((1, 2))).mean())
    with capsys.disabled():
        print(f"\n  W={W}, {len(boards)} boards: " + ", ".join(f"{k}: {v:.3f}" for k, v in shares.items()))
    for name, share in shares.items():
        assert share >= 0.10, (W, name, share)
