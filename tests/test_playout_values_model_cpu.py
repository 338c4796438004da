"""The product boundary of tron_playout_values, the maximin of tests/playout_support.py on matrices written by
hand, and the coverage of the inputs tests/test_gpu_playout_values.py plays, shown on the host model alone.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import playout_support as ps
import playout_values_support as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_bound_and_declared():
    """tron_playout_values is bound with its twelve arguments and declared in the header with the same twelve."""
    import tron.vec as tv
    nat = tv.nat                                                       # the ctypes binding
    res, args = nat.SIGNATURES["tron_playout_values"]
    vp = C.c_void_p
    assert res is C.c_int
    assert args == [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, vp, vp]
    with open(os.path.join(ROOT, "include", "tron_hip.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"\bint\s+tron_playout_values\s*\(([^)]*)\)\s*;", header)
    assert decl, "include/tron_hip.h does not declare tron_playout_values"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const int8_t *codes", "int64_t n", "int32_t side", "int32_t k_steps", "int32_t copies", "uint32_t seed",
                      "uint32_t stream_id", "uint64_t call", "int32_t *out_counts", "int32_t *out_steps", "int8_t *out_actions",
                      "void *stream"]
    assert hasattr(C.CDLL(nat.LIB_PATH), "tron_playout_values")


def counts_of(m):
    """counts [1, 4, 4, 4] whose wins of 1 minus wins of 2 are the matrix m[a1][a2]."""
    m = np.asarray(m)
    counts = np.zeros((1, 4, 4, 4), np.int32)
    counts[0, :, :, 1] = np.maximum(m, 0)
    counts[0, :, :, 2] = np.maximum(-m, 0)
    counts[0, :, :, 0] = 9 - np.abs(m)                                 # rows that sum to 9 copies
    return counts


def test_pick_by_hand():
    # a clear best move for each: row 2's worst case (1) beats every other row's; for player 2 (who wants m small)
    # column 1's worst case (max 2) beats every other column's
    m = [[3, -2, 5, 0],
         [-4, 1, 2, 6],
         [2, 1, 3, 4],
         [0, 2, -5, 7]]
    assert ps.pick(counts_of(m)).tolist() == [[2, 1]]
    # a full tie: UP for both
    assert ps.pick(counts_of(np.zeros((4, 4), int))).tolist() == [[0, 0]]
    assert ps.pick(counts_of(np.full((4, 4), -3))).tolist() == [[0, 0]]
    # a tie between two moves: the first of them (rows 1 and 3 both have worst case 2; columns 2 and 3 both worst case 4)
    m = [[1, 9, 4, 0],
         [5, 2, 4, 4],
         [0, 7, 3, 4],
         [6, 9, 2, 2]]
    assert ps.pick(counts_of(m)).tolist() == [[1, 2]]
    # player 2's negation: it minimises player 1's payoff, so where player 1 wins everything but column 3 it plays 3
    m = np.full((4, 4), 5)
    m[:, 3] = -5
    assert ps.pick(counts_of(m)).tolist() == [[0, 3]]
    # nothing played: a rejected board
    assert ps.pick(np.zeros((2, 4, 4, 4), np.int32)).tolist() == [[-1, -1], [-1, -1]]


def test_fan_out_index():
    """Index q = ((i * 16 + a1 * 4 + a2) * copies + j) holds board i and plays (a1, a2) first."""
    codes = np.arange(3 * 36, dtype=np.int8).reshape(3, 6, 6)
    copies = 3
    boards, tape = ps.fan_out(codes, 4, copies)
    assert boards.shape == (3 * 16 * copies, 6, 6) and tape.shape == (4, 3 * 16 * copies, 2)
    for i, a1, a2, j in ((0, 0, 0, 0), (1, 2, 3, 1), (2, 3, 3, 2), (2, 0, 1, 0)):
        q = (i * 16 + a1 * 4 + a2) * copies + j
        assert np.array_equal(boards[q], codes[i]) and tape[0, q].tolist() == [a1, a2]
    assert (tape[1:] < 0).all()
    assert ps.fan_out(codes, 0, copies)[1].shape == (0, 3 * 16 * copies, 2)


@pytest.mark.parametrize("W", pv.WIDTHS)
def test_gpu_inputs_reach_every_class(W):
    """On the model alone: the selected boards hold the three kinds of rejected board; at k_steps 7 all four classes
    occur; at W^2 nothing is unfinished; rejected boards give zeros and playable boards rows that sum to copies."""
    boards = pv.boards(W)
    assert boards.shape == (len(pv.SELECT), W + 2, W + 2) and set(pv.REJECTED) <= set(pv.SELECT)
    rejected = np.array([(b == 10).sum() != 1 or (b[1:-1, 1:-1] == 10).sum() != 1 for b in boards])
    assert all(rejected[pv.SELECT.index(i)] for i in pv.REJECTED) and 3 <= rejected.sum() < len(boards) // 4
    for copies in pv.COPIES:
        m = pv.model(W, copies)
        assert sorted(m) == sorted(pv.ks(W))
        for k, (counts, steps, actions) in m.items():
            assert counts.shape == (len(boards), 4, 4, 4) and steps.shape == (len(boards), 4, 4) and actions.shape == (len(boards), 2)
            assert (counts[rejected] == 0).all() and (steps[rejected] == 0).all() and (actions[rejected] == -1).all()
            assert (counts[~rejected].sum(3) == copies).all() and (actions[~rejected] >= 0).all()
        assert (m[0][0][~rejected, :, :, 3] == copies).all() and (m[0][1] == 0).all() and (m[0][2][~rejected] == 0).all()
        assert (m[7][0].sum((0, 1, 2)) > 0).all(), m[7][0].sum((0, 1, 2))
        assert m[W * W][0][..., 3].sum() == 0
        assert all(len(np.unique(m[W * W][2][~rejected, p])) > 1 for p in (0, 1))   # not every choice is the tie's UP
