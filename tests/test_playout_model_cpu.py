"""The host model of tron_playout_codes (tests/playout_support.py) against the episodes recorded from the reference, the
coverage of the inputs the GPU tests play, and the product boundary of the entry point.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
import playout_support as ps


def check_batch(boards, tape, length, winner, final, tag):
    (steps, win, codes), _ = ps.playout(boards, tape, k_steps=len(tape))[len(tape)]
    assert np.array_equal(steps, length), tag
    assert np.array_equal(win, winner), tag
    assert np.array_equal(codes, final), tag


@pytest.mark.parametrize("name", ["episodes_none_4", "episodes_none_10"])
def test_recorded_suffixes(name):
    """From the position after every step of every episode, the recorded actions lead to the recorded end: the
    remaining length, the winner and final_obs1."""
    g = load_golden(name)
    boards, tape, length, winner, final = ps.suffixes(g)
    assert len(boards) == len(g["actions"]) - (len(g["ep_off"]) - 1) and length.min() == 1
    check_batch(boards, tape, length, winner, final, name)


@pytest.mark.parametrize("name", ["episodes_none_4", "episodes_none_10", "episodes_none_24", "episodes_none_32",
                                  "episodes_uniform_10"])
def test_recorded_episodes_from_the_start(name):
    check_batch(*ps.starts(load_golden(name)), name)


def test_safe_draw_as_specified():
    """One draw spelled out by hand: the candidates in UP, RIGHT, DOWN, LEFT order, candidates[mulhi(u, c)] with u word
    p of the oracle's Philox at (index, step, call low, call high) under (seed, stream_id); UP without a candidate."""
    import oracle
    W, S = 5, 7
    grid = oracle.game_init(W, [2, 2, 0, 4])
    grid[2, 3] = 1                                                     # player 1 (cell [3][3] of the padded board): UP is taken
    grid[1, 4], grid[2, 5] = 3, 3                                      # player 2 at the corner: walled in
    codes = oracle.state_for_player(grid, 1)[None]
    key = dict(seed=123, stream_id=4, call=(5 << 32) | 6)
    m = ps.Playouts(codes, first_index=17, **key)
    m.t = 9
    got = m.safe_moves(np.array([[True, True]]))
    u = oracle.philox([17, 9, 6, 5], [123, 4])
    cand = [1, 2, 3]
    assert got[0, 0] == cand[(int(u[0]) * 3) >> 32] and got[0, 1] == 0 and m.boxed_in[0]


@pytest.mark.parametrize("W", ps.SOUP_WIDTHS)
def test_gpu_inputs_reach_every_class(W):
    """The boards and tapes of tests/test_gpu_playout.py meet every kind of ending on the model alone, at every width:
    a GPU test cannot pass by never meeting one.  Unfinished and all-finished both occur among the k_steps played."""
    boards, tapes, model = ps.soup(W)
    assert boards.shape == (ps.SOUP_N, W + 2, W + 2) and ps.SOUP_N % 64 != 0
    total = dict.fromkeys(ps.CLASSES, 0)
    for name in tapes:
        for k in ps.soup_ks(W):
            for cls, cnt in model[name][k][1].items():
                total[cls] += cnt
    assert all(total[cls] > 0 for cls in ps.CLASSES), total
    assert model["none"][1][1]["unfinished"] > 0
    assert all(model[name][W * W][1]["unfinished"] == 0 for name in tapes)
    steps = model["none"][W * W][0][0]
    assert steps.max() < W * W                                         # every playout finished before the last k_steps
    full = tapes["full"]
    assert full.min() == 0 and full.max() == 127 and (tapes["mixed"] < 0).any()


def test_entry_point_bound_and_host_tensors_refused():
    """tron_playout_codes is declared, exported and bound with its signature; playout_codes takes device tensors only."""
    import torch
    import tron.vec as tv
    nat = tv.nat                                                       # the ctypes binding
    res, args = nat.SIGNATURES["tron_playout_codes"]
    vp = C.c_void_p
    assert res is C.c_int
    assert args == [vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp]
    assert hasattr(C.CDLL(nat.LIB_PATH), "tron_playout_codes")
    with pytest.raises(nat.TronNativeError):
        tv.playout_codes(torch.ones(2, 6, 6, dtype=torch.int8), k_steps=3)
