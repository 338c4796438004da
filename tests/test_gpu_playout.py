"""tron_playout_codes / tron.vec.playout_codes / VecTron.playout on the GPU against the recorded episodes and the host
model of tests/playout_support.py.  Every comparison is exact.  tests/test_playout_model_cpu.py shows, without a GPU,
that the model reproduces the recorded episodes and that the boards and tapes used here meet every kind of ending."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from playout_gpu_support import mods, dev, run, same  # noqa: F401 (mods is a fixture)
import playout_support as ps
import rollout_support as rs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["episodes_none_4", "episodes_none_10"])
def test_recorded_suffixes(mods, name):
    """Every suffix of every recorded episode in one launch: the remaining length, the recorded winner and final_obs1.
    The tapes go on past each episode's end with moves that would be played if they were read."""
    boards, tape, length, winner, final = ps.suffixes(load_golden(name))
    same(run(mods, boards, tape, len(tape)), (length, winner, final), name)


@pytest.mark.parametrize("W", ps.SOUP_WIDTHS)
def test_soups_against_the_model(mods, W):
    """1 061 mid-game and rejected boards per width under a full tape over 0..127, no tape, and a mixed tape, at k_steps
    0, 1, 7 and W^2: steps, winner and the last position, rejected rows included."""
    boards, tapes, model = ps.soup(W)
    for name, tape in tapes.items():
        for k in ps.soup_ks(W):
            exp, tally = model[name][k]
            if name == "none" and k in (1, 7):
                assert tally["unfinished"] > 0                         # out_codes of an unfinished playout is compared
            same(run(mods, boards, tape, k, **ps.SOUP_KEY), exp, (W, name, k))


def test_draw_keying(mods):
    """The draws belong to (index, step, player, seed, stream_id, call) and to nothing else."""
    W, m = 10, 65
    boards, tapes, _ = ps.soup(W)
    twice = np.concatenate([boards[:m], boards[:m]])
    K = W * W
    # one board at two indices under one tape: one result
    tape = np.concatenate([tapes["full"][:, :m], tapes["full"][:, :m]], 1)
    got = run(mods, twice, tape, K, **ps.SOUP_KEY)
    same([g[:m] for g in got], [g[m:] for g in got], "same tape")
    # ... and with drawn moves each index follows its own draws, under every key
    base = ps.playout(twice, None, K, **ps.SOUP_KEY)[K][0]
    assert not np.array_equal(base[0][:m], base[0][m:])
    same(run(mods, twice, None, K, **ps.SOUP_KEY), base, "own index")
    for change in (dict(call=ps.SOUP_KEY["call"] + 1), dict(call=ps.SOUP_KEY["call"] + (1 << 32)), dict(seed=1),
                   dict(stream_id=6)):
        key = dict(ps.SOUP_KEY, **change)
        exp = ps.playout(twice, None, K, **key)[K][0]
        assert not np.array_equal(exp[0], base[0]), change
        same(run(mods, twice, None, K, **key), exp, change)
    # a launch of the first half agrees with the launch of the whole on its rows
    same(run(mods, twice[:m], None, K, **ps.SOUP_KEY), [g[:m] for g in base], "half")


@pytest.mark.parametrize("W", [5, 24])
def test_output_discipline(mods, W):
    """Every subset of NULL outputs; guard rows before and behind each output stay as they were; the boards and the
    outputs start at addresses that are no multiple of 16 (or of 4)."""
    tv, torch = mods
    nat = tv.nat                                                       # the ctypes binding
    boards, tapes, model = ps.soup(W)
    n, S, K = len(boards), W + 2, 7
    G, guard = S * S, 3
    exp = model["mixed"][K][0]
    raw = torch.zeros(n * G + 1, dtype=torch.int8, device="cuda")
    codes = raw[1:].view(n, S, S)                                      # an odd base address
    codes.copy_(dev(torch, boards))
    tape = dev(torch, tapes["mixed"])
    key = ps.SOUP_KEY
    for subset in range(8):
        outs = [torch.full((n + 2 * guard,) + shape, 77, dtype=dtype, device="cuda")
                for shape, dtype in (((), torch.int32), ((), torch.int8), ((S, S), torch.int8))]
        ptrs = [C.c_void_p(o[guard:].data_ptr()) if (subset >> j) & 1 else None for j, o in enumerate(outs)]
        nat.check(nat.lib().tron_playout_codes(nat.ptr(codes), n, S, K, nat.ptr(tape), key["seed"], key["stream_id"],
                                               key["call"], *ptrs, nat.stream_ptr()), "tron_playout_codes")
        torch.cuda.synchronize()
        for j, o in enumerate(outs):
            o = rs.np_(o)
            assert (o[:guard] == 77).all() and (o[-guard:] == 77).all(), (subset, j)
            if (subset >> j) & 1:
                assert np.array_equal(o[guard:-guard], exp[j]), (subset, j)
            else:
                assert (o == 77).all(), (subset, j)
    assert np.array_equal(rs.np_(codes), boards)                       # the input is only read


def test_handle_untouched(mods):
    """VecTron.playout reads the attached planes and leaves the env as it was: its twin, which ran no playout, holds the
    same state, planes and totals, and stays its twin over a further rollout."""
    tv, torch = mods
    N, W, copies, K = 2048, 24, 3, 40
    a, b = (tv.VecTron(N, W, seed=0xABC, rank=2) for _ in range(2))
    ta, tb = rs.new_totals(), rs.new_totals()
    tape = rs.make_tape(N, 30, salt=1)
    for env, tot in ((a, ta), (b, tb)):
        env.reset()
        env.rollout_actions(tape, tot)
    steps, winner, final = a.playout(k_steps=K, copies=copies, call=4, want_codes=True)
    rs.check_against_twin(rs.pull(a, ta), rs.pull(b, tb), "after the playout")
    # the playouts are playout_codes on the encoded boards, and the model's
    boards = tv.encode_codes(a.grid(), 1).repeat_interleave(copies, dim=0)
    assert torch.equal(boards.view(N, copies, -1)[:, 0], a.obs[:, 0].reshape(N, -1))
    key = dict(seed=0xABC, stream_id=2, call=4)
    got = tuple(rs.np_(t) for t in (steps, winner, final))
    same(tuple(rs.np_(t) for t in tv.playout_codes(boards, k_steps=K, want_codes=True, **key)), got, "playout_codes")
    same(got, ps.playout(rs.np_(boards), None, K, **key)[K][0], "model")
    assert (got[1] >= 0).any() and (got[1] == -1).any()
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

    def call(codes, n, side, k, out_codes=None):
        return L.tron_playout_codes(nat.ptr(codes), n, side, k, None, 1, 2, 3, None, None, nat.ptr(out_codes), nat.stream_ptr())

    c = torch.ones(4, 35, 35, dtype=torch.int8, device="cuda")
    assert call(c, 4, 5, 3) == nat.ERR_UNSUPPORTED and call(c, 4, 35, 3) == nat.ERR_UNSUPPORTED
    assert call(c, 4, 12, 3, out_codes=c) == nat.ERR_BAD_ARG
    assert call(c, -1, 12, 3) == nat.ERR_BAD_ARG and call(c, 4, 12, -1) == nat.ERR_BAD_ARG
    assert call(None, 4, 12, 3) == nat.ERR_BAD_ARG
    assert call(c, 0, 12, 3) == nat.OK and call(None, 0, 12, 3) == nat.OK
    steps, winner, final = tv.playout_codes(c[:0, :12, :12], k_steps=3, want_codes=True)
    assert steps.numel() == 0 and winner.numel() == 0 and final.numel() == 0
    env = tv.VecTron(4, 10, mode="ice")
    env.reset()
    with pytest.raises(ValueError):
        env.playout(k_steps=3)
    env.close()
    torch.cuda.synchronize()
