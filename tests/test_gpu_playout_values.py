"""tron_playout_values / tron.vec.playout_values / VecTron.playout_values / montecarlo_actions / play.rating's
"montecarlo" seat on the GPU, against the host model of tests/playout_support.py and against tron_playout_codes
itself.  Every comparison is exact.  tests/test_playout_values_model_cpu.py shows, without a GPU, that the boards used
here meet every class of ending."""
import ctypes as C

import numpy as np
import pytest

from playout_gpu_support import VALUES, mods, dev, run_values, same  # noqa: F401 (mods is a fixture)
import playout_support as ps
import playout_values_support as pv
import rollout_support as rs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("W", pv.WIDTHS)
def test_against_the_model(mods, W):
    """38 boards per width, rejected ones among them, at copies 1, 3, 4, 5 — four boards per wave, boards that straddle
    waves, one board per wave, a ragged last wave — and k_steps 0, 1, 7 and W^2: counts, steps and actions."""
    boards = pv.boards(W)
    for copies in pv.COPIES:
        model = pv.model(W, copies)
        for k in pv.ks(W):
            same(run_values(mods, boards, k, copies, **pv.KEY), model[k], (W, copies, k), VALUES)


@pytest.mark.parametrize("W", [5, 24])
def test_against_the_existing_kernel(mods, W):
    """The whole soup at copies 4, k_steps W^2: the tallies of playout_codes on the copied boards under the constructed
    tape and the same key."""
    tv, torch = mods
    boards = ps.soup(W)[0]
    n, copies, K = len(boards), 4, W * W
    codes = dev(torch, boards)
    q = torch.arange(n * 16 * copies, device="cuda")
    tape = torch.full((K, n * 16 * copies, 2), -1, dtype=torch.int8, device="cuda")
    move = (q // copies) % 16
    tape[0, :, 0], tape[0, :, 1] = (move >> 2).to(torch.int8), (move & 3).to(torch.int8)
    steps, winner, _ = tv.playout_codes(codes.repeat_interleave(16 * copies, dim=0), tape, K, **pv.KEY)
    exp = ps.tally(rs.np_(steps), rs.np_(winner), n, copies)
    got = run_values(mods, boards, K, copies, **pv.KEY)
    same(got, exp + (ps.pick(exp[0]),), W, VALUES)
    assert (got[0].reshape(n, -1).sum(1) == 0).sum() == len(range(5, n, 53))   # the soup's rejected boards, and no other
    assert all((got[0][..., c] > 0).any() for c in range(3)) and got[0][..., 3].sum() == 0


def test_keying(mods):
    """The draws belong to (index, step, player, seed, stream_id, call): each change of the key changes the counts and
    matches the model, and a launch of the first m boards is the first m rows of the whole."""
    W, copies, K = 10, 3, 100
    boards = pv.boards(W)
    base = pv.model(W, copies)[K]
    for change in (dict(call=pv.KEY["call"] + 1), dict(call=pv.KEY["call"] + (1 << 32)), dict(seed=1), dict(stream_id=6)):
        exp = pv.model(W, copies, **change)[K]
        assert not np.array_equal(exp[0], base[0]), change
        same(run_values(mods, boards, K, copies, **dict(pv.KEY, **change)), exp, change, VALUES)
    for m in (1, 7, 23):                                               # 23 * 48 playouts: the last wave is ragged
        same(run_values(mods, boards[:m], K, copies, **pv.KEY), [x[:m] for x in base], ("first", m), VALUES)


@pytest.mark.parametrize("W", [5, 10])
def test_output_discipline(mods, W):
    """Every subset of NULL outputs; guard rows of 77 before and behind each output stay as they were; the boards start
    at an odd address; the input is only read."""
    tv, torch = mods
    nat = tv.nat                                                       # the ctypes binding
    boards = pv.boards(W)
    n, S, K, copies, guard = len(boards), W + 2, 7, 3, 3
    exp = pv.model(W, copies)[K]
    raw = torch.zeros(n * S * S + 1, dtype=torch.int8, device="cuda")
    codes = raw[1:].view(n, S, S)                                      # an odd base address
    codes.copy_(dev(torch, boards))
    key = pv.KEY
    for subset in range(8):
        outs = [torch.full((n + 2 * guard,) + shape, 77, dtype=dtype, device="cuda")
                for shape, dtype in (((4, 4, 4), torch.int32), ((4, 4), torch.int32), ((2,), torch.int8))]
        ptrs = [C.c_void_p(o[guard:].data_ptr()) if (subset >> j) & 1 else None for j, o in enumerate(outs)]
        nat.check(nat.lib().tron_playout_values(nat.ptr(codes), n, S, K, copies, key["seed"], key["stream_id"], key["call"],
                                                *ptrs, nat.stream_ptr()), "tron_playout_values")
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            o = rs.np_(o)
            assert (o[:guard] == 77).all() and (o[-guard:] == 77).all(), (subset, j)
            if (subset >> j) & 1:
                assert np.array_equal(o[guard:-guard], exp[j]), (subset, j)
            else:
                assert (o == 77).all(), (subset, j)
    assert np.array_equal(rs.np_(codes), boards)


@pytest.mark.parametrize("copies", [1, 3, 4])
def test_forced_move(mods, copies):
    """Player 1 in a corner of a 6x6 board with its own trail to the right: DOWN is its one empty neighbour.  Player 2
    sits in the open.  After one step every other first move has lost against each of player 2's (safe) moves."""
    S = 8
    b = np.ones((S, S), np.int8)
    b[0], b[-1], b[:, 0], b[:, -1] = -1, -1, -1, -1
    b[1, 1], b[1, 2], b[1, 3] = 10, -2, -2
    b[4, 4], b[4, 5] = -10, -3                                         # its trail leaves UP, DOWN and LEFT free; RIGHT is not
    b2 = b.copy()
    b2[4, 5] = 1                                                       # ... and a player 2 with four safe moves
    counts, steps, actions = run_values(mods, np.stack([b, b2]), 1, copies, **pv.KEY)
    assert actions[:, 0].tolist() == [2, 2]
    for a1 in (0, 1, 3):
        assert (counts[1, a1, :, 2] == copies).all() and (counts[0, a1, [0, 2, 3], 2] == copies).all()
        assert counts[0, a1, 1].tolist() == [copies, 0, 0, 0]          # both crash: a draw
    assert (counts[1, 2, :, 3] == copies).all() and (counts[0, 2, [0, 2, 3], 3] == copies).all()
    assert counts[0, 2, 1].tolist() == [0, copies, 0, 0]
    assert (steps == copies).all()


def test_handle_untouched(mods):
    """VecTron.playout_values and montecarlo_actions read the env's boards and leave it as it was: its twin, which ran
    neither, holds the same state, planes and totals, and stays its twin over a further rollout."""
    tv, torch = mods
    N, W, copies, K = 300, 10, 2, 20
    a, b = (tv.VecTron(N, W, seed=0xABC, rank=2) for _ in range(2))
    ta, tb = rs.new_totals(), rs.new_totals()
    tape = rs.make_tape(N, 6, salt=1)
    for env, tot in ((a, ta), (b, tb)):
        env.reset()
        env.rollout_actions(tape, tot)
    got = a.playout_values(K, copies, call=4)
    mc = [a.montecarlo_actions(p, K, copies, call=4) for p in (1, 2)]
    mc_out = torch.full((N,), 77, dtype=torch.int8, device="cuda")
    assert a.montecarlo_actions(2, K, copies, call=4, out=mc_out) is mc_out
    rs.check_against_twin(rs.pull(a, ta), rs.pull(b, tb), "after the playouts")
    boards = tv.encode_codes(a.grid(), 1)
    key = dict(seed=0xABC, stream_id=2, call=4)
    got = tuple(rs.np_(t) for t in got)
    same(tuple(rs.np_(t) for t in tv.playout_values(boards, K, copies, **key)), got, "playout_values", VALUES)
    same(got, ps.values_model(rs.np_(boards), K, copies, **key), "model", VALUES)
    assert (got[0][..., 3] > 0).any() and (got[0][..., 1] > 0).any() and (got[0][..., 2] > 0).any()
    for p in (0, 1):
        assert mc[p].dtype == torch.int8 and np.array_equal(rs.np_(mc[p]), got[2][:, p])
    assert np.array_equal(rs.np_(mc_out), got[2][:, 1])
    full = rs.np_(a.montecarlo_actions(1, copies=1, call=5))           # the defaults: W^2 steps
    assert np.array_equal(full, rs.np_(tv.playout_values(boards, W * W, 1, seed=0xABC, stream_id=2, call=5)[2][:, 0]))
    tape2 = rs.make_tape(N, 40, salt=2)
    for env, tot in ((a, ta), (b, tb)):
        env.rollout_actions(tape2, tot)
    rs.check_against_twin(rs.pull(a, ta), rs.pull(b, tb), "after a further rollout")
    a.close()
    b.close()


def test_errors(mods):
    tv, torch = mods
    nat = tv.nat                                                       # the ctypes binding
    L = nat.lib()
    out = torch.full((4, 4, 4, 4), 77, dtype=torch.int32, device="cuda")

    def call(codes, n, side, k, copies=1):
        return L.tron_playout_values(nat.ptr(codes), n, side, k, copies, 1, 2, 3, nat.ptr(out), None, None, nat.stream_ptr())

    c = torch.ones(4, 35, 35, dtype=torch.int8, device="cuda")
    assert call(c, 4, 5, 3) == nat.ERR_UNSUPPORTED and call(c, 4, 35, 3) == nat.ERR_UNSUPPORTED
    assert call(None, 4, 12, 3) == nat.ERR_BAD_ARG
    assert call(c, -1, 12, 3) == nat.ERR_BAD_ARG and call(c, 4, 12, -1) == nat.ERR_BAD_ARG
    assert call(c, 4, 12, 3, copies=0) == nat.ERR_BAD_ARG and call(c, 4, 12, 3, copies=-2) == nat.ERR_BAD_ARG
    assert call(c, 1 << 27, 12, 3) == nat.ERR_BAD_ARG                  # n * 16 * copies = 2^31
    assert call(c, 4, 12, 3, copies=1 << 25) == nat.ERR_BAD_ARG
    assert call(c, 1 << 40, 12, 3) == nat.ERR_BAD_ARG
    assert call(c, 4, 12, 1 << 30, copies=2) == nat.ERR_BAD_ARG        # copies * k_steps = 2^31
    assert call(c, 0, 12, 3) == nat.OK and call(None, 0, 12, 3) == nat.OK
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                     # no call above wrote anything
    counts, steps, actions = tv.playout_values(c[:0, :12, :12], 3)
    assert counts.shape == (0, 4, 4, 4) and steps.shape == (0, 4, 4) and actions.shape == (0, 2)
    assert tv.playout_values(c[:2, :12, :12].contiguous(), 3, want_actions=False)[2] is None
    for bad in (dict(copies=0), dict(copies=1 << 27), dict(k_steps=-1), dict(k_steps=1 << 30, copies=2)):
        with pytest.raises(ValueError):
            tv.playout_values(c[:4, :12, :12].contiguous(), **dict(dict(k_steps=3), **bad))
    with pytest.raises(ValueError):
        tv.playout_values(c[:4, :12, :12].contiguous().to(torch.int32), 3)
    env = tv.VecTron(4, 10, mode="ice")
    env.reset()
    with pytest.raises(ValueError):
        env.playout_values(3)
    with pytest.raises(ValueError):
        env.montecarlo_actions(2)
    env.close()
    import play
    with pytest.raises(ValueError):
        play.rating(None, "montecarlo", n_games=4, slides=[0.0], width=10, gamemode="ice", verbose=False)
    torch.cuda.synchronize()


def test_rating_smoke(mods):
    """A player 1 that always goes UP against the Monte-Carlo seat: the winners are a partition of the games, and
    player 2 wins at least as many of them as it does when it always goes UP itself."""
    tv, torch = mods
    import play

    class Up:
        def act(self, x, env=None):
            return torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)

    games = 48
    args = dict(n_games=games, slides=[0.0], width=10, gamemode=None, verbose=False)
    (mc,), (up,) = play.rating(Up(), "montecarlo", **args), play.rating(Up(), Up(), **args)
    for r in (mc, up):
        assert r["p1_win"] + r["p2_win"] + r["draw"] == games and min(r["p1_win"], r["p2_win"], r["draw"]) >= 0
    assert mc["p2_win"] >= up["p2_win"]
