"""The host model of tron_search_codes (tests/search_support.py) without a GPU: it equals the literal recursive search on
boards of every width, the boards the GPU tests use tell every wrong model from the right one, and they hold what makes
the rules bite: wins, losses, draws and territory among the root values at every depth, and the planted positions."""
import numpy as np
import pytest

import search_support as ss
import territory_support as terr


def sample(W, count):
    """`count` boards of the width spread over the soup, the early and the planted boards, the last ones included."""
    b = ss.boards(W)
    at = np.unique(np.concatenate([np.linspace(0, len(b) - 1, count - 10).astype(int), np.arange(len(b) - 10, len(b))]))
    return b[at]


@pytest.mark.parametrize("W,plies,count", [(4, 1, 48), (4, 2, 48), (4, 3, 32), (5, 1, 48), (5, 2, 48), (5, 3, 32),
                                           (10, 1, 40), (10, 2, 24), (24, 1, 24), (24, 2, 12), (32, 1, 24), (32, 2, 12)])
def test_model_equals_the_literal_search(W, plies, count):
    boards = sample(W, count)
    values, actions = ss.model(boards, plies)
    assert values.dtype == np.int32 and values.shape == (len(boards), 2, 4) and actions.dtype == np.int8
    rejected = 0
    for i, board in enumerate(boards):
        lv, la = ss.literal(board, plies)
        assert values[i].tolist() == lv and actions[i].tolist() == la, (W, plies, i)
        rejected += la[0] < 0
    assert rejected < len(boards) // 2


@pytest.mark.parametrize("name", ss.WRONG_MODELS)
def test_the_boards_tell_every_wrong_model_from_the_right_one(name):
    """At width 5 alone, and at every depth at which the wrong model can depart from the right one at all."""
    for plies in ss.PLIES:
        boards = ss.deep_boards(5) if plies == 3 else ss.boards(5)
        right, wrong = ss.expected(5, plies), ss.model(boards, plies, **ss.WRONG_MODELS[name])
        differs = not (np.array_equal(right[0], wrong[0]) and np.array_equal(right[1], wrong[1]))
        assert differs == ss.can_differ(name, plies), (name, plies)


@pytest.mark.parametrize("W", (4, 5, 10))
@pytest.mark.parametrize("plies", ss.PLIES)
def test_wins_losses_draws_and_territory_occur_as_root_values(W, plies):
    values, actions = ss.expected(W, plies)
    ok = actions[:, 0] >= 0
    assert ok.any() and (~ok).any() and (values[~ok] == ss.REJECTED).all() and (actions[ok] >= 0).all() and (actions[ok] <= 3).all()
    boards = ss.deep_boards(W) if plies == 3 else ss.boards(W)
    for name, kind in zip(("win", "loss", "territory", "draw"), ss.kinds(values[ok], boards[ok])):
        assert kind.any(), name
    if W >= 5:                                                         # the draw by name: both players boxed in, no move safe
        box = len(values) - 10 + ss.PLANTED_NAMES.index("boxed in")
        assert (values[box] == 0).all() and actions[box].tolist() == [0, 0]


def test_planted_positions():
    """What each planted position is there for, on the 7 x 7 image itself."""
    boards = ss.planted(7)
    at = {name: i for i, name in enumerate(ss.PLANTED_NAMES)}
    one, two, three = (ss.model(boards, plies)[0] for plies in ss.PLIES)
    # heads two apart: RIGHT against LEFT is the same cell, a draw, and it bounds both moves' worst case from above
    assert one[at["two apart"], 0, 1] == 0 and one[at["two apart"], 1, 3] == 0
    # heads side by side: each player's move onto the other's head is unsafe and loses at once
    assert one[at["adjacent"], 0, 1] == -2048 and one[at["adjacent"], 1, 3] == -2048
    # one safe move into a dead end two deep: territory at 1 and 2 plies, a loss after two joint moves at 3
    assert [v[at["dead end"], 0, 1] for v in (one, two, three)] == [-7, -7, -2046]
    assert (three[at["dead end"], 1, [0, 2, 3]] == 2046).all()
    # V_1 + V_2 != 0: the two maximins are no zero-sum pair
    assert any(v[i, 0].max() + v[i, 1].max() != 0 for v in (two, three) for i in range(len(boards)))
    # the swapped copies: the same values with the players exchanged
    for v in (one, two, three):
        assert np.array_equal(v[5:], v[:5, ::-1])
