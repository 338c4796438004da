"""The host model of tron_reach_codes (tests/reach_support.py): it equals a literal queue BFS on the hand boards of every side
and on a slice of every width's boards, agrees with the territory model where the two overlap, its fill bound is never below
the true longest walk on the 4 x 4 boards, and the inputs of the GPU tests tell every wrong model from the right one."""
import numpy as np
import pytest

import reach_support as rch
import territory_support as terr


@pytest.mark.parametrize("S", rch.SIDES)
def test_model_equals_literal_on_hand_boards(S):
    boards = rch.hand_boards(S)
    counts, dist = rch.model(boards)
    for i, b in enumerate(boards):
        lc, ld = rch.literal(b)
        assert list(counts[i]) == lc and np.array_equal(dist[i], ld), (S, i)
    assert (counts[-2:] == -1).all() and (dist[-2:] == -1).all() and (counts[:-2] >= 0).all()
    # the split arena: above the wall only player 1 is in the last interior column, below it only player 2
    d = dist[5]
    assert (d[0, 2:S // 2, S - 2] > 0).all() and (d[1, 2:S // 2, S - 2] == -1).all()
    assert (d[1, S // 2 + 1:S - 2, S - 2] > 0).all() and (d[0, S // 2 + 1:S - 2, S - 2] == -1).all()


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_model_equals_literal_on_a_slice_of_the_boards(W):
    boards = rch.boards(W)
    counts, dist = rch.expected(W)
    for i in list(range(0, len(boards), 13)) + [len(boards) - 2, len(boards) - 1]:
        lc, ld = rch.literal(boards[i])
        assert list(counts[i]) == lc and np.array_equal(dist[i], ld), (W, i)


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_agrees_with_the_territory_model(W):
    """opp + same are territory's first counts, a rejected row is -1 throughout, the owner plane follows from the two
    distance planes, depth is the greatest value of a plane, and the bound and the first count disagree often enough
    for the judges to differ."""
    boards = rch.boards(W)
    counts, dist = rch.expected(W)
    tc, owner = terr.model(boards)
    bad = tc[:, 0] < 0
    assert bad.any() and (counts[bad] == -1).all() and (dist[bad] == -1).all() and (counts[~bad] >= 0).all()
    c = counts[~bad]
    assert np.array_equal(c[:, rch.OPP1] + c[:, rch.SAME1], tc[~bad, terr.FIRST1])
    assert np.array_equal(c[:, rch.OPP2] + c[:, rch.SAME2], tc[~bad, terr.FIRST2])
    assert np.array_equal(rch.owner_from_dist(dist, boards), owner)
    assert np.array_equal(dist[~bad].max((2, 3)), c[:, 6:])
    assert np.array_equal((dist[~bad] == 0).sum((2, 3)), np.ones((len(c), 2)))
    assert np.array_equal((dist[~bad] > 0).sum((2, 3)), tc[~bad, 4:6])
    assert (c[:, rch.FILL1] <= tc[~bad, terr.FIRST1]).all() and (c[:, rch.FILL1] != tc[~bad, terr.FIRST1]).sum() >= 250
    assert (rch.winner(counts) != terr.winner(tc)).sum() >= 7


def test_fill_is_never_below_the_longest_walk():
    """Every playable 4 x 4 board, both players: the true longest walk inside first_p by exhaustive search (16 cells at
    most) against fill_p.  The bound is met with equality on most boards and is not always met."""
    boards = rch.boards(4)
    counts, _ = rch.expected(4)
    met = total = 0
    seen = {}
    for i in np.nonzero(counts[:, 0] >= 0)[0]:
        for p in range(2):
            cells, head = rch.first_cells(boards[i], p)
            key = (frozenset(cells), head)
            if key not in seen:
                seen[key] = rch.longest_walk(cells, head)
            assert seen[key] <= counts[i, 4 + p], (i, p, seen[key], counts[i])
            met += seen[key] == counts[i, 4 + p]
            total += 1
    assert total > 5000 and total // 2 < met < total


def test_serpentine():
    """fill1 is the corridor's length: every cell of it in one walk.  The depths are what the int16 planes are for."""
    for S, depth in ((18, 133), (26, 297), (34, 525)):
        board = terr.serpentine(S)
        counts, dist = rch.model(board[None])
        cells = int((board == 1).sum())
        assert counts[0, rch.FILL1] == cells == counts[0, rch.OPP1] + counts[0, rch.SAME1]
        assert list(counts[0, [rch.OPP2, rch.SAME2, rch.FILL2, rch.DEPTH2]]) == [0, 0, 0, 0]
        assert counts[0, rch.DEPTH1] == depth == dist[0, 0].max() and (dist[0, 1] >= 0).sum() == 1


def test_winner():
    counts = np.array([[3, 2, 0, 0, 5, 0, 4, 0], [2, 3, 9, 9, 4, 18, 1, 1], [4, 4, 1, 1, 2, 2, 0, 0], [-1] * 8, [0] * 8], np.int32)
    assert list(rch.winner(counts)) == [1, 2, 0, -2, 0]


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_inputs_tell_every_wrong_model(W, capsys):
    """A condition on the inputs: every wrong model departs from the model on at least one board in ten, the saturating
    ones on the serpentines, and only where a board that deep exists."""
    boards = rch.boards(W)
    counts, dist = rch.expected(W)
    hits = {}
    for name, kw in rch.WRONG_MODELS.items():
        wc, wd = rch.model(boards, **kw)
        hits[name] = int(((wc != counts).any(1) | (wd != dist).any((1, 2, 3))).sum())
    with capsys.disabled():
        print(f"\n  W={W}, {len(boards)} boards: " + ", ".join(f"{k}: {v}" for k, v in hits.items()))
    for name, hit in hits.items():
        if "saturate" in rch.WRONG_MODELS[name]:
            assert hit == (2 if rch.can_differ(name, W) else 0), (W, name, hit)
        else:
            assert hit >= len(boards) // 10, (W, name, hit)


@pytest.mark.parametrize("S", (18, 26, 32, 34))
def test_hand_boards_tell_the_saturating_models(S):
    """The serpentine among the hand boards and the arenas of tests/test_gpu_reach.py: 127 is passed at side 18, 255 at 26."""
    boards = rch.hand_boards(S) if S in rch.SIDES else terr.serpentine(S)[None]
    counts, dist = rch.model(boards)
    for sat in (127, 255):
        wc, wd = rch.model(boards, saturate=sat)
        assert ((wc != counts).any() or (wd != dist).any()) == (counts[:, 6:].max() > sat), (S, sat)
    assert counts[:, 6:].max() > (127 if S < 26 else 255)
