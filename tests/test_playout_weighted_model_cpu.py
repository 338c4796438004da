"""The host model of tron_playout_weighted_codes / tron_playout_weighted_values (tests/playout_support.py with weights): the
cumulative pick on hand-written matrices, the weight vectors that are the uniform draw against the mode-None and sliding
models, the coverage of the inputs the GPU tests play, the product boundary of the two entries and the checks of
weights= that need no device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import playout_support as ps
import playout_slide_support as pss
import playout_values_support as pv
import playout_weighted_support as pw


def test_cumulative_pick_by_hand():
    """x at 0, at every running sum minus one and at every running sum picks the candidate the rule names; u is chosen as
    the smallest word with mulhi(u, T) == x."""
    def u_of(x, T):
        u = -((-x << 32) // T)                                         # ceil(x * 2^32 / T)
        assert (u * T) >> 32 == x and (x == 0 or ((u - 1) * T) >> 32 == x - 1) and u < 1 << 32
        return u

    # four candidates of weights 3, 0, 5, 2: running sums 3, 3, 8, 10; candidate 1 is never taken
    w, free = [3, 0, 5, 2], [True] * 4
    expected = {0: 0, 2: 0, 3: 2, 7: 2, 8: 3, 9: 3}
    for x, move in expected.items():
        got, T, cnt = ps.weighted_pick(w, free, u_of(x, 10))
        assert (int(got), int(T), int(cnt)) == (move, 10, 4), x
    # UP and DOWN are no candidates, whatever their room weighs: running sums 0, 4, 4, 5
    w, free = [9, 4, 9, 1], [False, True, False, True]
    for x, move in {0: 1, 3: 1, 4: 3}.items():
        got, T, cnt = ps.weighted_pick(w, free, u_of(x, 5))
        assert (int(got), int(T), int(cnt)) == (move, 5, 2), x
    # T = 1020, the largest sum: x = T - 1 at the largest word, and the running sums 255, 510, 765
    w = [255] * 4
    assert ((0xFFFFFFFF * 1020) >> 32) == 1019
    for x, move in {0: 0, 254: 0, 255: 1, 509: 1, 510: 2, 764: 2, 765: 3, 1019: 3}.items():
        assert int(ps.weighted_pick(w, free=[True] * 4, u=u_of(x, 1020))[0]) == move, x
    assert int(ps.weighted_pick(w, [True] * 4, 0xFFFFFFFF)[0]) == 3
    # T == 0: candidates[mulhi(u, cnt)] — the second of three at u = 2^32 / 3 rounded up; no candidate: UP
    got, T, cnt = ps.weighted_pick([0, 0, 0, 0], [True, False, True, True], u_of(1, 3))
    assert (int(got), int(T), int(cnt)) == (2, 0, 3)
    assert int(ps.weighted_pick([0, 0, 0, 0], [True, False, True, True], u_of(1, 3) - 1)[0]) == 0
    assert int(ps.weighted_pick([7, 7, 7, 7], [False] * 4, 0xDEADBEEF)[0]) == 0
    # a single non-zero weight on one candidate: the move does not depend on u
    for u in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        assert int(ps.weighted_pick([0, 0, 6, 0], [True] * 4, u)[0]) == 2
    # equal weights are the uniform pick at every u of a sweep, for every set of candidates
    us = np.arange(0, 1 << 32, 0x01000193, dtype=np.uint64)
    for mask in range(16):
        free = np.array([[bool(mask >> a & 1) for a in range(4)]] * len(us))
        plain = ps.weighted_pick(np.ones(4), free, us)[0]
        for w in (7, 255):
            assert np.array_equal(ps.weighted_pick(np.full(4, w), free, us)[0], plain), (mask, w)


def test_rooms_by_hand():
    """The room of each move on the hand-built boards: 0 into the dead end, 3 into the open; a neighbour off the image is
    not EMPTY."""
    boards, player, dead, opened = pw.dead_end_boards()
    assert len(boards) == 16
    m = ps.Playouts(boards, weights=(1, 1, 1, 1))
    free, room = m.rooms(np.arange(len(boards)))
    for i in range(len(boards)):
        p = player[i] - 1
        assert free[i, p].sum() == 2 and free[i, p, dead[i]] and free[i, p, opened[i]], i
        assert room[i, p, dead[i]] == 0 and room[i, p, opened[i]] == 3, i
    leaky = pw.border_boards()[-2:]
    free, room = ps.Playouts(leaky, weights=(1, 1, 1, 1)).rooms(np.arange(2))
    # head at (1, 1) under an EMPTY border: UP and LEFT are on the ring, two of their neighbours are ring cells
    assert free[0, 0].tolist() == [True, True, True, True] and room[0, 0].tolist() == [2, 3, 3, 2]
    assert free[1, 0].tolist() == [True, True, True, True] and room[1, 0].tolist() == [3, 2, 2, 3]


@pytest.mark.parametrize("W", [4, 5, 10])
def test_equal_weights_are_the_uniform_draw(W):
    """At (1,1,1,1), (0,0,0,0), (7,7,7,7) and (255,255,255,255) the model is playout_support.playout / the sliding model
    on the soups, under every tape and k_steps."""
    boards, tapes, plain = ps.soup(W)
    _, _, rates, slide = pss.soup(W)
    for weights in pw.UNIFORM_EQUAL:
        for name, tape in tapes.items():
            got = ps.playout(boards, tape, ks=ps.soup_ks(W), rates=None, weights=weights, **ps.SOUP_KEY)
            got_slide = ps.playout(boards, tape, ks=ps.soup_ks(W), rates=rates, weights=weights, **ps.SOUP_KEY)
            for k in ps.soup_ks(W):
                for g, e in zip(got[k][0] + got_slide[k][0], plain[name][k][0] + slide[name][k][0]):
                    assert g.dtype == e.dtype and np.array_equal(g, e), (W, weights, name, k)
                assert got[k][1]["not_uniform"] == 0 and got_slide[k][1]["not_uniform"] == 0
                assert all(got_slide[k][1][cls] == cnt for cls, cnt in slide[name][k][1].items())


def test_values_model_at_equal_weights():
    """The values model at equal weights is the one without weights, and the sliding one its composition."""
    W, copies = 5, 3
    for k, exp in pv.model(W, copies).items():
        got = ps.values_model(pv.boards(W), k, copies, weights=(7, 7, 7, 7), **pv.KEY)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), k
    got = pw.values_soup_model(W, (1, 8, 4, 2), "slide", copies)[W * W]
    played = ps.decode(pv.boards(W))[2]
    assert (got[0][played].sum(3) == copies).all() and (got[0][~played] == 0).all() and (got[2][~played] == -1).all()


@pytest.mark.parametrize("W", [10, 32])
def test_gpu_inputs_reach_every_class(W):
    """The inputs of tests/test_gpu_playout_weighted.py meet, on the model alone, every kind of drawn move a weight
    vector can meet (playout_weighted_support.classes_of: a vector without a 0 never skips a move and never falls back)."""
    for weights in pw.WEIGHTED:
        total = dict.fromkeys(pw.DRAW_CLASSES, 0)
        for rule in pw.RULES:
            for tape in pw.TAPES:
                model = pw.soup_model(W, weights, rule, tape)
                for cls in pw.DRAW_CLASSES:
                    total[cls] += model[W * W][1][cls]                 # the counts run on over the k_steps
                assert model[W * W][1]["unfinished"] == 0
        assert all(total[cls] > 0 for cls in pw.classes_of(weights)), (weights, total)
        assert all(total[cls] == 0 for cls in pw.DRAW_CLASSES if cls not in pw.classes_of(weights)), (weights, total)
    assert pw.classes_of((0, 255, 0, 1)) == pw.DRAW_CLASSES and pw.classes_of((3, 0, 0, 0)) == pw.DRAW_CLASSES


def differing(W, weights, rule, tape, k):
    """bool [N]: the boards whose (steps, winner) under `weights` are not the uniform draw's in one GPU case."""
    got, plain = pw.soup_model(W, weights, rule, tape)[k][0], pw.soup_model(W, (1, 1, 1, 1), rule, tape)[k][0]
    return (got[0] != plain[0]) | (got[1] != plain[1])


@pytest.mark.parametrize("W", [10, 32])
def test_a_kernel_that_ignores_the_weights_fails(W):
    """A condition on the inputs (as RATE_SEEDS is on the rates), pinned here: in the case of drawn moves played to the end
    (no tape, k_steps W^2), under mode None's rule and under the sliding rule alike, the model's (steps, winner) at each
    non-uniform weight vector are not the uniform model's on at least one board in ten of the width's N boards.  The soup
    alone does not give that ((3,0,0,0) departs from the uniform draw only beside a dead end: 4 % of the soup's boards of
    width 32), which is why the inputs hold the planted boards.  Under the mixed tape few moves are drawn; there, and at
    every shorter k_steps where anything is drawn, some board differs.  The shares on the model, mode None / sliding:
    width 10 (1,8,4,2) 46.0 / 33.9 %, (0,255,0,1) 52.2 / 46.0 %, (3,0,0,0) 26.3 / 19.7 %; width 32 26.6 / 22.4 %,
    27.4 / 28.5 %, 17.9 / 16.8 %."""
    assert len(pw.soup_boards(W)) == pw.N == ps.SOUP_N + pw.EXTRA_N and ps.decode(pw.soup_boards(W)[ps.SOUP_N:])[2].all()
    for weights in pw.WEIGHTED:
        for rule in pw.RULES:
            share = differing(W, weights, rule, "none", W * W).mean()
            print(W, weights, rule, f"{share:.3f}")
            assert share >= 0.1, (W, weights, rule, share)
            assert differing(W, weights, rule, "mixed", W * W).any() and differing(W, weights, rule, "none", 7).any()


def test_entry_points_bound_and_weights_checked():
    """The two weighted entries are declared in the header, exported and bound with their signatures; weights= is
    checked, each fault with its own message, before anything needs a device; weights=None goes on to the existing
    entries (which refuse a host tensor)."""
    import torch
    import tron.vec as tv
    nat = tv.nat                                                       # the ctypes binding
    vp, u32 = C.c_void_p, C.c_uint32
    res, args = nat.SIGNATURES["tron_playout_weighted_codes"]
    assert res is C.c_int
    assert args == [vp, C.c_int64, C.c_int32, C.c_int32, vp, vp, vp, u32, u32, u32, C.c_uint64, vp, vp, vp, vp]
    res, args = nat.SIGNATURES["tron_playout_weighted_values"]
    assert res is C.c_int
    assert args == [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, u32, u32, u32, C.c_uint64, vp, vp, vp, vp]
    lib = C.CDLL(nat.LIB_PATH)
    assert hasattr(lib, "tron_playout_weighted_codes") and hasattr(lib, "tron_playout_weighted_values")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tron_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int tron_playout_weighted_codes(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, "
            "const int8_t *actions, const double *rates, const float *uniforms, uint32_t weights, uint32_t seed, "
            "uint32_t stream_id, uint64_t call, int32_t *out_steps, int8_t *out_winner, int8_t *out_codes, "
            "void *stream);") in flat
    assert ("int tron_playout_weighted_values(const int8_t *codes, int64_t n, int32_t side, int32_t k_steps, int32_t copies, "
            "const double *rates, uint32_t weights, uint32_t seed, uint32_t stream_id, uint64_t call, "
            "int32_t *out_counts, int32_t *out_steps, int8_t *out_actions, void *stream);") in flat
    assert nat.ABI_VERSION == 13 and "#define TRON_ABI_VERSION 13" in re.sub(r"[ \t]+", " ", header)
    assert tv.HUG_WEIGHTS in pw.CANDIDATES and tv._packed_weights((1, 8, 4, 2), "x") == 0x02040801 == pw.packed((1, 8, 4, 2))
    boards = torch.ones(2, 6, 6, dtype=torch.int8)
    for call in (lambda **kw: tv.playout_codes(boards, k_steps=3, **kw), lambda **kw: tv.playout_values(boards, 3, **kw)):
        for bad, exc, text in (((1, 2, 3), ValueError, "four"), ((1, 2, 3, 4, 5), ValueError, "four"),
                               ((1, 2, 3, 256), ValueError, "0..255"), ((-1, 2, 3, 4), ValueError, "0..255"),
                               ((1.0, 2, 3, 4), TypeError, "ints"), (("1", 2, 3, 4), TypeError, "ints"),
                               ((True, 2, 3, 4), TypeError, "ints"), (5, TypeError, "sequence")):
            with pytest.raises(exc, match=text):
                call(weights=bad)
        for good in ((1, 8, 4, 2), [0, 0, 0, 0], np.array([255, 0, 1, 2]), None):
            with pytest.raises(nat.TronNativeError):                   # checked and handed on: the host tensor is refused
                call(weights=good)
