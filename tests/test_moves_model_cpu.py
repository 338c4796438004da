"""The host model of tron_moves_codes (tests/moves_support.py): it equals a literal queue BFS on the hand boards of every side
and on a slice of every width's boards, keeps the invariants that tie it to the territory model, its fill bound is never
below the true longest walk on small boards, and the inputs of the GPU tests tell every wrong model from the right one."""
import numpy as np
import pytest

import moves_support as mv
import reach_support as rch
import territory_support as terr


def assert_literal(boards, moves, actions, rows, tag):
    for i in rows:
        lm, la = mv.literal(boards[i])
        assert np.array_equal(np.array(lm, np.int32), moves[i]) and la == list(actions[i]), (tag, i, lm, moves[i], la, actions[i])


@pytest.mark.parametrize("S", rch.SIDES)
def test_model_equals_literal_on_hand_boards(S):
    boards = rch.hand_boards(S)
    moves, actions = mv.model(boards)
    assert_literal(boards, moves, actions, range(len(boards)), S)
    assert (moves[-2:] == -1).all() and (actions[-2:] == -1).all() and (actions[:-2] >= 0).all()
    # the serpentine: player 1's one safe move leads through every cell of the corridor, player 2 has none
    corridor = int((boards[7] == 1).sum())
    assert mv.safe(moves[7]).sum() == 1 and list(moves[7, 0, 1]) == [corridor] * 3 and list(actions[7]) == [1, 0]


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_model_equals_literal_on_a_slice_of_the_boards(W):
    boards = mv.boards(W)
    moves, actions = mv.expected(W)
    assert_literal(boards, moves, actions, list(range(0, len(boards), 11)) + [len(boards) - 2, len(boards) - 1], W)


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_invariants(W):
    """For every playable row and safe move: 1 <= first + [d_q(t) = 1] <= room <= reach_p, fill <= room, and the greatest
    room of a player is reach_p whenever all its safe targets lie in one component.  A player has 0..4 safe moves, and a
    rejected row is -1 throughout."""
    boards = mv.boards(W)[::3 if W > 10 else 1]
    moves, actions, fl = mv.model(boards, details=True)
    tc = terr.model(boards)[0]
    bad = tc[:, 0] < 0
    assert bad.any() and (moves[bad] == -1).all() and (actions[bad] == -1).all() and (actions[~bad] >= 0).all()
    safe = mv.safe(moves)
    assert np.array_equal(safe, fl["target"].any((3, 4))) and not safe[bad].any()
    assert set(np.unique(safe[~bad].sum(-1))) == {0, 1, 2, 3, 4}
    assert (moves[~safe] == -1).all()
    room, fill, first = (moves[..., k] for k in range(3))
    beside = np.stack([(fl["target"][:, p] & (fl["d"][:, 1 - p] == 1)[:, None]).any((2, 3)) for p in range(2)], 1)
    reach = np.broadcast_to(tc[:, 4:6, None], room.shape)
    assert (1 <= (first + beside)[safe]).all() and ((first + beside)[safe] <= room[safe]).all()
    assert beside[safe].any() and (first[safe] < room[safe]).sum() > 1000
    assert (room[safe] <= reach[safe]).all() and (fill[safe] <= room[safe]).all() and (fill[safe] >= 1).all()
    # one component: every safe target of the player is reached by the flood from each of its safe targets
    targets = (fl["target"] & safe[..., None, None]).any(2)                                   # [n, 2, S, S]
    inside = (fl["reached"] | ~targets[:, :, None]).all((3, 4)) | ~safe                       # [n, 2, 4]
    one = inside.all(-1) & safe.any(-1)
    assert one.sum() > 500 and (~one & safe.any(-1)).sum() > 20
    assert np.array_equal(room.max(-1)[one], tc[:, 4:6][one])
    # an action is a safe move wherever there is one, UP where there is none
    a = actions[~bad].astype(np.int64)
    took = np.take_along_axis(safe[~bad], a[..., None], -1)[..., 0]
    assert np.array_equal(took, safe[~bad].any(-1)) and (a[~safe[~bad].any(-1)] == 0).all()


def test_fill_is_never_below_the_longest_walk():
    """Small boards of width 4 and 5, every safe move of both players: the true longest walk that starts on t and stays
    in the reached cells, by exhaustive search, against fill.  The bound is met on most moves and not on all."""
    met = total = 0
    seen = {}
    for W, count in ((4, 48), (5, 36)):
        boards = mv.boards(W)
        moves, _, fl = mv.model(boards[:400], details=True)
        rows = [i for i in range(400) if moves[i, :, :, mv.ROOM].max() >= 1 and moves[i, :, :, mv.ROOM].max() <= 14][:count]
        assert len(rows) == count
        for i in rows:
            for p in range(2):
                for a in range(4):
                    if moves[i, p, a, mv.ROOM] < 0:
                        continue
                    t = tuple(np.argwhere(fl["target"][i, p, a])[0])
                    cells = frozenset(map(tuple, np.argwhere(fl["reached"][i, p, a]))) - {t}
                    if (cells, t) not in seen:
                        seen[(cells, t)] = 1 + rch.longest_walk(cells, t)              # t is the first cell of the walk
                    walk = seen[(cells, t)]
                    assert walk <= moves[i, p, a, mv.FILL], (W, i, p, a, walk, moves[i, p, a])
                    met += walk == moves[i, p, a, mv.FILL]
                    total += 1
    assert total > 150 and total // 2 < met < total


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_inputs_tell_every_wrong_model(W, capsys):
    """A condition on the inputs: every wrong model departs from the model on at least one board of the width's set.  The
    models that keep the floods are run on all of it from one set of floods; the three that flood differently on every
    fifth board and the planted ones (the doors and the rings are what they are about), which is enough."""
    boards = mv.boards(W)
    moves, actions = mv.expected(W)
    given = mv.floods(boards)
    part = np.r_[0:len(boards) - 4 * terr.PLANT_N - 2:5, len(boards) - 4 * terr.PLANT_N - 2:len(boards)]
    hits = {}
    for name, kw in mv.WRONG_MODELS.items():
        if set(kw) & {"through_own_head", "through_other_head", "open_border"}:
            wm, wa = mv.model(boards[part], **kw)
            hits[name] = int(((wm != moves[part]).any((1, 2, 3)) | (wa != actions[part]).any(1)).sum())
        else:
            wm, wa = mv.model(boards, given=given, **kw)
            hits[name] = int(((wm != moves).any((1, 2, 3)) | (wa != actions).any(1)).sum())
    with capsys.disabled():
        print(f"\n  W={W}, {len(boards)} boards: " + ", ".join(f"{k}: {v}" for k, v in hits.items()))
    for name, hit in hits.items():
        assert hit >= 1, (W, name)
    # the picks part on the actions alone, and where safe moves of one player lead into different room
    rooms = np.where(mv.safe(moves), moves[..., mv.ROOM], 0)
    assert ((rooms.max(-1) != np.where(mv.safe(moves), rooms, 1 << 20).min(-1)) & mv.safe(moves).any(-1)).sum() > 300
