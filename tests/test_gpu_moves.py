"""tron_moves_codes / tron.vec.moves_codes / safe_moves / VecTron.moves / VecTron.lookahead_actions and play.rating's
"lookahead" seat, on the GPU, against the host model of tests/moves_support.py.  Every comparison is exact.
tests/test_moves_model_cpu.py shows, without a GPU, that the model equals a literal BFS on the boards used here and that
these boards tell every wrong model from the right one."""
import ctypes as C

import numpy as np
import pytest

from playout_gpu_support import mods, dev, same  # noqa: F401 (mods is a fixture)
import moves_support as mv
import playout_support as ps
import reach_support as rch
import rollout_support as rs
import territory_support as terr

pytestmark = pytest.mark.gpu

MOVES = ("moves", "actions")
MOVE_FILL, ACTION_FILL = 0x5A5A5A5A, 0x77


def run_moves(mods, boards, want_actions=True):
    """moves_codes on host arrays -> (moves, actions | None) as host arrays."""
    tv, torch = mods
    moves, actions = tv.moves_codes(dev(torch, boards), want_actions=want_actions)
    torch.cuda.synchronize()
    return rs.np_(moves), (None if actions is None else rs.np_(actions))


def check(mods, boards, exp, tag):
    """Both outputs, the moves alone, and safe_moves on them."""
    tv, torch = mods
    same(run_moves(mods, boards), exp, tag, MOVES)
    moves, actions = run_moves(mods, boards, want_actions=False)
    assert actions is None and np.array_equal(moves, exp[0]), tag
    safe = tv.safe_moves(dev(torch, exp[0]))
    assert safe.dtype == torch.bool and np.array_equal(rs.np_(safe), exp[0][..., 0] >= 0), tag


@pytest.mark.parametrize("W", terr.WIDTHS)
def test_moves_and_actions_equal_the_model(mods, W):
    """The soup, the early and the planted boards of the width, rejected boards and the serpentines included."""
    check(mods, mv.boards(W), mv.expected(W), W)


@pytest.mark.parametrize("S", rch.SIDES)
def test_hand_built_boards_at_the_instantiation_boundaries(mods, S):
    """8, 16 and 32 rows per board with 32-bit masks up to side 32, 64 rows and 64-bit masks at sides 33 and 34.  The split
    arena's door (board 6) is in the last interior column: mask bit 31 / 32 at sides 33 / 34, and player 1's way DOWN."""
    boards = rch.hand_boards(S)
    exp = mv.model(boards)
    assert boards[6][S // 2, S - 2] == 1 and exp[0][6, 0, 2, mv.ROOM] > exp[0][5, 0, 2, mv.ROOM] > 0
    check(mods, boards, exp, S)


@pytest.mark.parametrize("S", (8, 16, 32, 34))
def test_serpentine_next_to_empty_arenas(mods, S):
    """One long corridor (more than 255 levels at sides 32 and 34) among empty arenas that finish after a few levels.  Sides
    8, 16 and 32 put 8, 4 and 2 boards in a wave, so the corridor and the arenas share one.  The corridor's one safe move
    has room = fill = first = its whole length."""
    snake, plain = terr.serpentine(S), terr.arena(S, (1, 1), (S - 2, S - 2))
    boards = np.stack([snake if i in (1, 6, 19) else plain for i in range(21)])
    exp = mv.model(boards)
    length = int((snake == 1).sum())
    assert mv.safe(exp[0][1]).sum() == 1 and list(exp[0][1, 0, 1]) == [length] * 3 and (S < 32 or length > 256)
    check(mods, boards, exp, S)


@pytest.mark.parametrize("W", (4, 10, 24))
def test_a_ring_of_ones_between_ordinary_boards(mods, W):
    """Every other board of a wave has a border ring of all 1: it counts as the same board with a wall ring, and its
    neighbours' rows are what they are without it."""
    boards = ps.soup_boards(W)[:96]
    exp = mv.model(boards)
    for odd in (1, 0):
        mixed = boards.copy()
        mixed[odd::2] = terr.ring_of_ones(boards[odd::2])
        assert (mixed != boards).any()
        same(run_moves(mods, mixed), exp, (W, odd), MOVES)


def raw(mods, codes_ptr, n, side, moves, actions, row=1):
    """The C entry on raw pointers; moves / actions are the guarded buffers or None, the outputs start at their row `row`."""
    tv, torch = mods
    nat = tv.nat
    mp = None if moves is None else C.c_void_p(moves.data_ptr() + row * 24 * 4)
    ap = None if actions is None else C.c_void_p(actions.data_ptr() + row * 2)
    rc = nat.lib().tron_moves_codes(codes_ptr, n, side, mp, ap, nat.stream_ptr())
    torch.cuda.synchronize()
    return rc


def guarded(torch, n):
    moves = torch.full((n + 2, 2, 4, 3), MOVE_FILL, dtype=torch.int32, device="cuda")
    actions = torch.full((n + 2, 2), ACTION_FILL, dtype=torch.int8, device="cuda")
    return moves, actions


def check_guarded(moves, actions, n, exp, want_moves=True, want_actions=True):
    m, a = rs.np_(moves), rs.np_(actions)
    assert (m[0] == MOVE_FILL).all() and (m[n + 1] == MOVE_FILL).all() and (a[0] == ACTION_FILL).all() and (a[n + 1] == ACTION_FILL).all()
    assert np.array_equal(m[1:n + 1], exp[0][:n]) if want_moves else (m == MOVE_FILL).all()
    assert np.array_equal(a[1:n + 1], exp[1][:n]) if want_actions else (a == ACTION_FILL).all()


@pytest.mark.parametrize("W", (5, 10, 32))
def test_batch_sizes_and_null_outputs(mods, W):
    """n of 1, 63, 64, 65 and 203 (a last wave partly empty at every side), sentinel rows round both outputs, each output
    NULL in turn."""
    tv, torch = mods
    S = W + 2
    exp = tuple(x[1000:1203] for x in mv.expected(W))
    codes = dev(torch, mv.boards(W)[1000:1203])
    for n in (1, 63, 64, 65, 203):
        for want_moves, want_actions in ((True, True), (True, False), (False, True)):
            moves, actions = guarded(torch, n)
            rc = raw(mods, tv.nat.ptr(codes), n, S, moves if want_moves else None, actions if want_actions else None)
            assert rc == tv.nat.OK
            check_guarded(moves, actions, n, exp, want_moves, want_actions)


@pytest.mark.parametrize("W", (5, 10, 32))
def test_misaligned_boards_at_the_end_of_the_allocation(mods, W):
    """codes 1, 5 and 15 bytes past a 16-byte boundary, the last board ending with its allocation."""
    tv, torch = mods
    S, n = W + 2, 37
    boards = mv.boards(W)[1040:1040 + n]
    exp = tuple(x[1040:1040 + n] for x in mv.expected(W))
    for off in (1, 5, 15):
        buf = torch.empty(off + n * S * S, dtype=torch.int8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        codes = buf[off:].view(n, S, S)
        codes.copy_(dev(torch, boards))
        moves, actions = guarded(torch, n)
        assert raw(mods, C.c_void_p(codes.data_ptr()), n, S, moves, actions) == tv.nat.OK
        check_guarded(moves, actions, n, exp)
        assert np.array_equal(rs.np_(codes), boards)
        got = tv.moves_codes(codes)
        same((rs.np_(got[0]), rs.np_(got[1])), exp, (W, off), MOVES)


def test_refused_arguments_write_nothing(mods):
    tv, torch = mods
    nat = tv.nat
    n, S = 8, 12
    codes = dev(torch, mv.boards(10)[:n])
    cases = [(nat.ptr(codes), -1, S, nat.ERR_BAD_ARG), (nat.ptr(codes), 2 ** 31, S, nat.ERR_BAD_ARG), (None, n, S, nat.ERR_BAD_ARG),
             (nat.ptr(codes), n, 5, nat.ERR_UNSUPPORTED), (nat.ptr(codes), n, 35, nat.ERR_UNSUPPORTED),
             (nat.ptr(codes), -1, 40, nat.ERR_BAD_ARG), (None, n, 40, nat.ERR_BAD_ARG),     # told before an unsupported side
             (None, 0, S, nat.OK), (nat.ptr(codes), 0, S, nat.OK)]
    keep = codes.clone()
    for cp, nn, side, want in cases:
        moves, actions = guarded(torch, n)
        assert raw(mods, cp, nn, side, moves, actions) == want, (nn, side)
        check_guarded(moves, actions, n, None, False, False)
    assert raw(mods, nat.ptr(codes), n, S, None, None) == nat.OK       # both outputs NULL: nothing to do
    assert torch.equal(codes, keep)
    with pytest.raises(ValueError):
        tv.moves_codes(codes.to(torch.int32))
    with pytest.raises(nat.TronNativeError):
        tv.moves_codes(codes.cpu())


def test_env_methods_leave_the_env_alone(mods):
    """VecTron.moves and lookahead_actions against the functions on the env's codes, after a short rollout."""
    tv, torch = mods
    W, N = 10, 96
    env = tv.VecTron(N, W, seed=0xABE, rank=1)
    env.reset()
    env.rollout_actions(rs.make_tape(N, 5, salt=2), rs.new_totals())
    before = env.grid().clone()
    p1 = env._p1_codes().clone()
    exp = mv.model(rs.np_(p1))
    moves, actions = env.moves()
    assert np.array_equal(rs.np_(moves), exp[0]) and np.array_equal(rs.np_(actions), exp[1]) and (exp[1] >= 0).any()
    only, none = env.moves(want_actions=False)
    assert none is None and torch.equal(only, moves)
    for a, b in zip(tv.moves_codes(p1), (moves, actions)):
        assert torch.equal(a, b)
    for player in (1, 2):
        got = env.lookahead_actions(player)
        assert got.dtype == torch.int8 and got.shape == (N,) and got.is_contiguous() and torch.equal(got, actions[:, player - 1])
        out = torch.full((N,), 9, dtype=torch.int8, device="cuda")
        assert env.lookahead_actions(player, out=out) is out and torch.equal(out, got)
    for bad in (0, 3):
        with pytest.raises(ValueError):
            env.lookahead_actions(bad)
    assert torch.equal(env.grid(), before)
    env.close()


@pytest.mark.parametrize("W", (5, 24))
def test_cross_checks_on_the_device(mods, W):
    """Against territory_codes and the bytes themselves, on the device: a playable board's greatest room is no more than the
    player's reach, and a move is safe exactly where the byte at the target is 1 strictly inside the border."""
    tv, torch = mods
    S = W + 2
    codes = dev(torch, mv.boards(W))
    moves, _ = tv.moves_codes(codes)
    counts, _ = tv.territory_codes(codes)
    ok = counts[:, 0] >= 0
    assert bool(ok.any()) and bool((~ok).any()) and bool((moves[~ok] == -1).all())
    assert bool((moves[ok][..., 0].max(-1).values <= counts[ok][:, 4:6]).all())
    inside = torch.zeros_like(codes, dtype=torch.bool)
    inside[:, 1:-1, 1:-1] = codes[:, 1:-1, 1:-1] == 1
    flat = inside[ok].reshape(-1, S * S)
    for p, byte in enumerate((10, -10)):
        at = (codes[ok] == byte).reshape(-1, S * S).to(torch.int8).argmax(1)
        for a, (dr, dc) in enumerate(mv.DELTAS):
            target = at + dr * S + dc                                  # a head is strictly inside: the target is on the image
            assert torch.equal(tv.safe_moves(moves[ok])[:, p, a], flat.gather(1, target[:, None])[:, 0]), (W, p, a)


def test_rating_smoke(mods):
    """A player 1 that always goes UP against the lookahead seat in mode None: what the other seats return in shape and
    type, the winners a partition of the games.  No score is asserted."""
    tv, torch = mods
    import play

    class Up:
        def act(self, x, env=None):
            return torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)

    res = play.rating(Up(), model2="lookahead", n_games=64, width=10, gamemode=None, verbose=False)
    assert len(res) == 13 and all(set(r) == {"slide", "p1_win", "p2_win", "draw", "p1_rate"} for r in res)
    for r in res:
        assert all(isinstance(r[k], int) for k in ("p1_win", "p2_win", "draw")) and isinstance(r["p1_rate"], float)
        assert r["p1_win"] + r["p2_win"] + r["draw"] == 64 and min(r["p1_win"], r["p2_win"], r["draw"]) >= 0
