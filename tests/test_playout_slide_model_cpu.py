"""The host model of tron_playout_slide_codes (tests/playout_support.py with rates) against the sliding episodes recorded
from the reference and against the mode-None model, the coverage of the inputs the GPU tests play, and the product
boundary of the two entry points.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
import playout_support as ps
import playout_slide_support as pss


def check_batch(boards, tape, uniforms, rates, length, winner, final, tag):
    (steps, win, codes), _ = ps.playout(boards, tape, k_steps=len(tape), rates=rates, uniforms=uniforms)[len(tape)]
    assert np.array_equal(steps, length), tag
    assert np.array_equal(win, winner), tag
    assert np.array_equal(codes, final), tag


@pytest.mark.parametrize("name", ["episodes_ice_4", "episodes_temper_4"])
def test_recorded_suffixes(name):
    """From the position after every step of every sliding episode, the recorded actions and uniforms under the recorded
    rates lead to the recorded end: the remaining length, the winner and final_obs1."""
    g = load_golden(name)
    batch = pss.suffixes(g)
    assert len(batch[0]) == len(g["actions"]) - (len(g["ep_off"]) - 1) and batch[4].min() == 1
    assert g["consumed"].any()
    check_batch(*batch, name)


@pytest.mark.parametrize("name", ["episodes_ice_4", "episodes_ice_10", "episodes_ice_24", "episodes_temper_4",
                                  "episodes_temper_10", "episodes_temper_24"])
def test_recorded_episodes_from_the_start(name):
    check_batch(*pss.starts(load_golden(name)), name)


@pytest.mark.parametrize("W", ps.SOUP_WIDTHS)
def test_never_sliding_is_mode_none(W):
    """With all rates -1 the model is playout_support.playout on the mode-None soups, under every tape and k_steps."""
    boards, tapes, plain = ps.soup(W)
    rates = np.full((len(boards), 2), -1.0)
    for name, tape in tapes.items():
        got = ps.playout(boards, tape, ks=ps.soup_ks(W), rates=rates, **ps.SOUP_KEY)
        for k in ps.soup_ks(W):
            for g, e in zip(got[k][0], plain[name][k][0]):
                assert np.array_equal(g, e), (W, name, k)
            assert all(got[k][1][cls] == cnt for cls, cnt in plain[name][k][1].items())
            assert not any(got[k][1][cls] for cls in ps.SLIDE_CLASSES)


def test_uniform_as_specified():
    """u of (index, step, player) is (word[2 + p] >> 8) * 2^-24 of the block at (index, step, call low, call high) under
    (seed, stream_id), and the decision is float64(u) <= rate: a rate just below u does not slide, u itself does."""
    import oracle
    codes = oracle.state_for_player(oracle.game_init(5, [2, 2, 0, 4]), 1)[None]
    key = dict(seed=123, stream_id=4, call=(5 << 32) | 6)
    words = oracle.philox([17, 9, 6, 5], [123, 4])
    u = ps.philox_uniform(words[2:])
    assert u.dtype == np.float32 and np.array_equal(u, ((words[2:] >> 8) / 2.0 ** 24).astype(np.float32))
    for rates, exp in (([float(u[0]), np.nextafter(np.float64(u[1]), -1.0)], [True, False]),
                       ([np.nextafter(np.float64(u[0]), -1.0), float(u[1])], [False, True]),
                       ([float("nan"), 1.5], [False, True]), ([-0.0, -1e-300], [bool(u[0] == 0), False])):
        m = ps.Playouts(codes, np.array([rates]), first_index=17, **key)
        m.t = 9
        assert m.slides(np.array([True])).tolist() == [exp]


def test_hand_built_boards():
    """Four one-step boards that force the orderings of a step: the model gives the endings worked out by hand and meets
    both ordering classes, a double slide, a slide onto the border and a slide onto a trail."""
    boards, tape, rates, steps, winner, final = pss.hand_built()
    (got, tally), = ps.playout(boards, tape, k_steps=1, rates=rates).values()
    for g, e in zip(got, (steps, winner, final)):
        assert g.dtype == e.dtype and np.array_equal(g, e)
    assert tally["p1_dies_on_p2_tile"] == 1 and tally["p2_target_filled"] == 1
    assert tally["slide"] == 4 and tally["both_slid"] == 1 and tally["slide_to_border"] == 1 and tally["slide_to_trail"] == 1


@pytest.mark.parametrize("W", ps.SOUP_WIDTHS)
def test_gpu_inputs_reach_every_class(W):
    """The boards, tapes and rates of tests/test_gpu_playout_slide.py meet every class on the model alone — every kind of
    ending and, from width 10 on, every kind of sliding step: a GPU test cannot pass by never meeting one."""
    boards, tapes, rates, model = pss.soup(W)
    assert rates.shape == (ps.SOUP_N, 2) and np.isnan(rates).any()
    assert all((rates == v).any() for v in pss.RATE_VALUES if v == v)
    assert ((rates > 0) & (rates < 1) & ~np.isin(rates, pss.RATE_VALUES)).any()
    total = dict.fromkeys(pss.CLASSES, 0)
    for name in tapes:
        for k in ps.soup_ks(W):
            for cls, cnt in model[name][k][1].items():
                total[cls] += cnt
    need = pss.CLASSES if W >= 10 else ps.CLASSES + ("slide", "both_slid", "slide_to_border", "slide_to_trail")
    assert all(total[cls] > 0 for cls in need), total
    assert model["none"][1][1]["unfinished"] > 0
    assert all(model[name][W * W][1]["unfinished"] == 0 for name in tapes)


def test_entry_points_bound_and_host_tensors_refused():
    """The two sliding entries are declared, exported and bound with their signatures; playout_codes and playout_values
    check rates and uniforms before anything is launched and take device tensors only."""
    import torch
    import tron.vec as tv
    nat = tv.nat                                                       # the ctypes binding
    vp, u32 = C.c_void_p, C.c_uint32
    res, args = nat.SIGNATURES["tron_playout_slide_codes"]
    assert res is C.c_int
    assert args == [vp, C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, u32, u32, C.c_uint64, vp, vp, vp, vp]
    res, args = nat.SIGNATURES["tron_playout_slide_values"]
    assert res is C.c_int
    assert args == [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, u32, u32, C.c_uint64, vp, vp, vp, vp]
    lib = C.CDLL(nat.LIB_PATH)
    assert hasattr(lib, "tron_playout_slide_codes") and hasattr(lib, "tron_playout_slide_values")
    boards = torch.ones(2, 6, 6, dtype=torch.int8)
    rates = torch.zeros(2, 2, dtype=torch.float64)
    with pytest.raises(TypeError):
        tv.playout_codes(boards, k_steps=3, rates=rates.float())
    with pytest.raises(TypeError):
        tv.playout_values(boards, 3, rates=[[0.0, 0.0]] * 2)
    with pytest.raises(ValueError):
        tv.playout_codes(boards, k_steps=3, rates=rates[:1])
    with pytest.raises(ValueError):
        tv.playout_values(boards, 3, rates=torch.zeros(2, 4, dtype=torch.float64)[:, ::2])
    with pytest.raises(ValueError):
        tv.playout_codes(boards, k_steps=3, uniforms=torch.zeros(3, 2, 2))          # uniforms without rates
    with pytest.raises(TypeError):
        tv.playout_codes(boards, k_steps=3, rates=rates, uniforms=torch.zeros(3, 2, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        tv.playout_codes(boards, k_steps=4, rates=rates, uniforms=torch.zeros(3, 2, 2))
    with pytest.raises(nat.TronNativeError):
        tv.playout_codes(boards, k_steps=3, rates=rates)
    with pytest.raises(nat.TronNativeError):
        tv.playout_values(boards, 3, rates=rates)
