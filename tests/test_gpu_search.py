"""tron_search_codes / tron.vec.search_codes / VecTron.search / VecTron.search_actions and play.rating's "search" seat, on
the GPU, against the host model of tests/search_support.py and, without any host model, against playout_codes and
territory_codes on the device.  Every comparison is exact.  tests/test_search_model_cpu.py shows, without a GPU, that the
model equals a literal recursive search on the boards used here and that these boards tell every wrong model from the
right one."""
import ctypes as C

import numpy as np
import pytest

from playout_gpu_support import dev, same
import playout_support as ps
import reach_support as rch
import rollout_support as rs
import search_support as ss
import territory_support as terr

pytestmark = pytest.mark.gpu

SEARCH = ("values", "actions")
VALUE_FILL, ACTION_FILL = 0x5A5A5A5A, 0x77


@pytest.fixture(scope="module")
def mods():
    tv, _ = rs.gpu_modules()
    import torch
    assert callable(tv.search_codes) and tv.SEARCH_REJECTED == ss.REJECTED and tv.nat.lib().tron_search_codes
    return tv, torch


def run_search(mods, boards, plies, want_actions=True):
    """search_codes on host arrays -> (values, actions | None) as host arrays."""
    tv, torch = mods
    values, actions = tv.search_codes(dev(torch, boards), plies=plies, want_actions=want_actions)
    torch.cuda.synchronize()
    return rs.np_(values), (None if actions is None else rs.np_(actions))


def check(mods, boards, plies, exp, tag):
    """Both outputs, and the values alone."""
    same(run_search(mods, boards, plies), exp, tag, SEARCH)
    values, actions = run_search(mods, boards, plies, want_actions=False)
    assert actions is None and np.array_equal(values, exp[0]), tag


@pytest.mark.parametrize("plies", (1, 2))
@pytest.mark.parametrize("W", terr.WIDTHS)
def test_values_and_actions_equal_the_model(mods, W, plies):
    """The soup, the early and the planted boards of the width, rejected boards, the serpentines and the positions planted
    for the search included."""
    check(mods, ss.boards(W), plies, ss.expected(W, plies), (W, plies))


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_three_plies_equal_the_model(mods, W):
    """A few hundred boards at widths 4, 5 and 10, a few dozen at 24 and 32."""
    boards = ss.deep_boards(W)
    assert len(boards) >= (200 if W <= 10 else 24)
    check(mods, boards, 3, ss.expected(W, 3), W)


@pytest.mark.parametrize("plies", ss.PLIES)
@pytest.mark.parametrize("S", rch.SIDES)
def test_hand_built_boards_at_the_instantiation_boundaries(mods, S, plies):
    """8, 16 and 32 rows per board with 32-bit masks up to side 32, 64 rows and 64-bit masks at sides 33 and 34.  The split
    arena's door (board 6) is in the last interior column: mask bit 31 / 32 at sides 33 / 34, and the way DOWN of player
    1, which stands in that column."""
    boards = rch.hand_boards(S)
    exp = ss.model(boards, plies)
    assert boards[6][S // 2, S - 2] == 1 and boards[6][1, S - 2] == 10
    assert plies > 1 or not np.array_equal(exp[0][6], exp[0][5])       # one ply deep the door's bit decides values
    check(mods, boards, plies, exp, (S, plies))


@pytest.mark.parametrize("plies", ss.PLIES)
@pytest.mark.parametrize("S", (8, 16, 32, 34))
def test_serpentine_next_to_empty_arenas(mods, S, plies):
    """One long corridor (more than 255 levels at sides 32 and 34) among empty arenas that finish after a few levels.  Sides
    8, 16 and 32 put 8, 4 and 2 boards in a wave, so the corridor and the arenas share one.  The corridor's player 2 is
    sealed in: player 1 wins the first joint move by its one safe direction."""
    snake, plain = terr.serpentine(S), terr.arena(S, (1, 1), (S - 2, S - 2))
    boards = np.stack([snake if i in (1, 6, 19) else plain for i in range(21)])
    exp = ss.model(boards, plies)
    assert exp[0][1, 0].tolist() == [0, 2048, 0, 0] and (exp[0][1, 1] == -2048).all() and (abs(exp[0][0]) < 2046).any()
    check(mods, boards, plies, exp, (S, plies))


@pytest.mark.parametrize("W", (4, 10, 24))
def test_a_ring_of_ones_between_ordinary_boards(mods, W):
    """Every other board of a wave has a border ring of all 1: it counts as the same board with a wall ring, and its
    neighbours' rows are what they are without it."""
    boards = ss.boards(W)[:96]
    exp = tuple(x[:96] for x in ss.expected(W, 2))
    for odd in (1, 0):
        mixed = boards.copy()
        mixed[odd::2] = terr.ring_of_ones(boards[odd::2])
        assert (mixed != boards).any()
        same(run_search(mods, mixed, 2), exp, (W, odd), SEARCH)


def raw(mods, codes_ptr, n, side, plies, values, actions, row=1):
    """The C entry on raw pointers; values / actions are the guarded buffers or None, the outputs start at their row `row`."""
    tv, torch = mods
    nat = tv.nat
    vp = None if values is None else C.c_void_p(values.data_ptr() + row * 8 * 4)
    ap = None if actions is None else C.c_void_p(actions.data_ptr() + row * 2)
    rc = nat.lib().tron_search_codes(codes_ptr, n, side, plies, vp, ap, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc


def guarded(torch, n):
    values = torch.full((n + 2, 2, 4), VALUE_FILL, dtype=torch.int32, device="cuda")
    actions = torch.full((n + 2, 2), ACTION_FILL, dtype=torch.int8, device="cuda")
    return values, actions


def check_guarded(values, actions, n, exp, want_values=True, want_actions=True):
    v, a = rs.np_(values), rs.np_(actions)
    assert (v[0] == VALUE_FILL).all() and (v[n + 1] == VALUE_FILL).all() and (a[0] == ACTION_FILL).all() and (a[n + 1] == ACTION_FILL).all()
    assert np.array_equal(v[1:n + 1], exp[0][:n]) if want_values else (v == VALUE_FILL).all()
    assert np.array_equal(a[1:n + 1], exp[1][:n]) if want_actions else (a == ACTION_FILL).all()


@pytest.mark.parametrize("W,plies", ((5, 1), (5, 2), (10, 2), (32, 2)))
def test_batch_sizes_and_null_outputs(mods, W, plies):
    """n of 1, 63, 64, 65 and 203 (a last wave partly empty at every side), sentinel rows round both outputs, each output
    NULL in turn."""
    tv, torch = mods
    S = W + 2
    exp = tuple(x[1000:1203] for x in ss.expected(W, plies))
    codes = dev(torch, ss.boards(W)[1000:1203])
    for n in (1, 63, 64, 65, 203):
        for want_values, want_actions in ((True, True), (True, False), (False, True)):
            values, actions = guarded(torch, n)
            rc = raw(mods, tv.nat.ptr(codes), n, S, plies, values if want_values else None, actions if want_actions else None)
            assert rc == tv.nat.OK
            check_guarded(values, actions, n, exp, want_values, want_actions)


@pytest.mark.parametrize("W", (5, 10, 32))
def test_misaligned_boards_at_the_end_of_the_allocation(mods, W):
    """codes 1, 5 and 15 bytes past a 16-byte boundary, the last board ending with its allocation."""
    tv, torch = mods
    S, n = W + 2, 37
    boards = ss.boards(W)[1040:1040 + n]
    exp = tuple(x[1040:1040 + n] for x in ss.expected(W, 2))
    for off in (1, 5, 15):
        buf = torch.empty(off + n * S * S, dtype=torch.int8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        codes = buf[off:].view(n, S, S)
        codes.copy_(dev(torch, boards))
        values, actions = guarded(torch, n)
        assert raw(mods, C.c_void_p(codes.data_ptr()), n, S, 2, values, actions) == tv.nat.OK
        check_guarded(values, actions, n, exp)
        assert np.array_equal(rs.np_(codes), boards)
        got = tv.search_codes(codes, plies=2)
        same((rs.np_(got[0]), rs.np_(got[1])), exp, (W, off), SEARCH)


def test_refused_arguments_write_nothing(mods):
    tv, torch = mods
    nat = tv.nat
    n, S = 8, 12
    codes = dev(torch, ss.boards(10)[:n])
    cp = nat.ptr(codes)
    cases = [(cp, -1, S, 2, nat.ERR_BAD_ARG), (cp, 2 ** 31, S, 2, nat.ERR_BAD_ARG), (None, n, S, 2, nat.ERR_BAD_ARG),
             (cp, n, 5, 2, nat.ERR_UNSUPPORTED), (cp, n, 35, 2, nat.ERR_UNSUPPORTED),
             (cp, n, S, 0, nat.ERR_UNSUPPORTED), (cp, n, S, 4, nat.ERR_UNSUPPORTED),
             (cp, -1, 40, 2, nat.ERR_BAD_ARG), (None, n, 40, 2, nat.ERR_BAD_ARG),       # told before an unsupported side
             (cp, -1, S, 4, nat.ERR_BAD_ARG), (None, n, S, 0, nat.ERR_BAD_ARG),         # and before unsupported plies
             (None, 0, S, 2, nat.OK), (cp, 0, S, 2, nat.OK)]
    keep = codes.clone()
    for ptr, nn, side, plies, want in cases:
        values, actions = guarded(torch, n)
        assert raw(mods, ptr, nn, side, plies, values, actions) == want, (nn, side, plies)
        check_guarded(values, actions, n, None, False, False)
    assert raw(mods, cp, n, S, 2, None, None) == nat.OK                # both outputs NULL: nothing to do
    assert torch.equal(codes, keep)
    for plies in (0, 4):
        with pytest.raises(nat.TronNativeError):
            tv.search_codes(codes, plies=plies)
    with pytest.raises(ValueError):
        tv.search_codes(codes.to(torch.int32))
    with pytest.raises(nat.TronNativeError):
        tv.search_codes(codes.cpu())


@pytest.mark.parametrize("plies", (1, 2))
@pytest.mark.parametrize("W", (5, 10))
def test_device_cross_check_without_the_model(mods, W, plies):
    """Every one of the 16 ** plies joint lines of 64 playable boards played by playout_codes under a tape, the lines that
    are still open judged by territory_codes on the last position; W_p of a line from (steps, winner, first1 - first2)
    alone; the min / max fold on the host."""
    tv, torch = mods
    boards = ss.boards(W)
    boards = np.concatenate([boards[:200][terr.model(boards[:200])[0][:, 0] >= 0][:54], boards[-10:]])
    n, L = len(boards), 16 ** plies
    assert n == 64
    line = np.arange(L)
    digits = [(line >> (2 * (2 * plies - 1 - j))) & 3 for j in range(2 * plies)]      # a_1, b_1, a_2, b_2 of a line
    tape = np.stack([np.stack([np.tile(digits[2 * t], n), np.tile(digits[2 * t + 1], n)], 1) for t in range(plies)]).astype(np.int8)
    fanned = dev(torch, boards).repeat_interleave(L, dim=0)
    steps, winner, final = tv.playout_codes(fanned, dev(torch, tape), plies, want_codes=True)
    counts, _ = tv.territory_codes(final)
    torch.cuda.synchronize()
    steps, winner, counts = (rs.np_(t).astype(np.int64) for t in (steps, winner, counts))
    assert set(np.unique(winner)) == {-1, 0, 1, 2} and (counts[winner == -1, 0] >= 0).all() and (steps[winner == -1] == plies).all()
    decided = ss.DECIDED - (steps - 1)
    w1 = np.where(winner == -1, counts[:, 0] - counts[:, 1], np.where(winner == 0, 0, np.where(winner == 1, decided, -decided)))
    w1, w2 = w1.reshape((n,) + (4,) * (2 * plies)), (-w1).reshape((n,) + (4,) * (2 * plies))
    if plies == 2:                                                     # V_p of the children: max over the own move of the min
        w1, w2 = w1.min(4).max(3), w2.min(3).max(3)
    u = np.stack([w1.min(2), w2.min(1)], 1)
    values, actions = run_search(mods, boards, plies)
    assert np.array_equal(values, u.astype(np.int32)) and np.array_equal(actions, u.argmax(-1).astype(np.int8)), (W, plies)


def test_env_methods_leave_the_env_alone(mods):
    """VecTron.search and search_actions against the function on the env's codes, after a short rollout."""
    tv, torch = mods
    W, N = 10, 96
    env = tv.VecTron(N, W, seed=0xABE, rank=1)
    env.reset()
    env.rollout_actions(rs.make_tape(N, 5, salt=2), rs.new_totals())
    before = env.grid().clone()
    p1 = env._p1_codes().clone()
    for plies in ss.PLIES:
        exp = ss.model(rs.np_(p1), plies)
        values, actions = env.search(plies=plies)
        assert np.array_equal(rs.np_(values), exp[0]) and np.array_equal(rs.np_(actions), exp[1]) and (exp[1] >= 0).any()
        only, none = env.search(plies=plies, want_actions=False)
        assert none is None and torch.equal(only, values)
        for a, b in zip(tv.search_codes(p1, plies=plies), (values, actions)):
            assert torch.equal(a, b)
        for player in (1, 2):
            got = env.search_actions(player, plies=plies)
            assert got.dtype == torch.int8 and got.shape == (N,) and got.is_contiguous() and torch.equal(got, actions[:, player - 1])
            out = torch.full((N,), 9, dtype=torch.int8, device="cuda")
            assert env.search_actions(player, plies=plies, out=out) is out and torch.equal(out, got)
    assert torch.equal(env.search()[0], env.search(plies=2)[0])        # the default depth
    for bad in (0, 3):
        with pytest.raises(ValueError):
            env.search_actions(bad)
    assert torch.equal(env.grid(), before)
    env.close()


def test_rating_smoke(mods):
    """A player 1 that always goes UP against the search seat in mode None: what the other seats return in shape and type,
    the winners a partition of the games.  No score is asserted."""
    tv, torch = mods
    import play

    class Up:
        def act(self, x, env=None):
            return torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)

    res = play.rating(Up(), model2="search", search_plies=2, n_games=64, width=10, gamemode=None, verbose=False)
    assert len(res) == 13 and all(set(r) == {"slide", "p1_win", "p2_win", "draw", "p1_rate"} for r in res)
    for r in res:
        assert all(isinstance(r[k], int) for k in ("p1_win", "p2_win", "draw")) and isinstance(r["p1_rate"], float)
        assert r["p1_win"] + r["p2_win"] + r["draw"] == 64 and min(r["p1_win"], r["p2_win"], r["draw"]) >= 0
