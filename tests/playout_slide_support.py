"""The inputs of the sliding-playout tests (tests/test_playout_slide_model_cpu.py, tests/test_gpu_playout_slide.py): rates
for playout_support's soups, hand-built boards that force the orderings of one step, and the recorded sliding episodes
as batches.  The model is playout_support's, given rates.  A plain module, imported by name; nothing here needs a GPU."""
import numpy as np

import oracle
import playout_support as ps

CLASSES = ps.SLIDE_CLASSES + ps.CLASSES
RATE_VALUES = (-1.0, 0.0, 0.03, 0.15, 0.5, 1.0, 1.5, float("nan"))

# ---- the soups: playout_support's boards and action tapes, with rates of their own -----------------------------------
RATE_SEEDS = {4: 21, 5: 22, 10: 23, 24: 24, 32: 34}             # chosen so that widths 10 and up meet every class


def soup_rates(W, n=ps.SOUP_N, seed=None):
    """float64 [n, 2]: per board and player one of RATE_VALUES or a uniform random rate in [0, 1), independently."""
    rs = np.random.RandomState(RATE_SEEDS[W] if seed is None else seed)
    pick = rs.randint(0, len(RATE_VALUES) + 1, (n, 2))
    table = np.array(RATE_VALUES + (0.0,), np.float64)
    return np.where(pick == len(RATE_VALUES), rs.random_sample((n, 2)), table[pick])


@ps.once
def soup(W):
    """(boards, tapes, rates, {tape name: playout(...) at soup_ks(W)}) of width W under playout_support.SOUP_KEY and
    Philox uniforms."""
    boards, tapes, _ = ps.soup(W)
    rates = soup_rates(W)
    model = {name: ps.playout(boards, tape, ks=ps.soup_ks(W), rates=rates, **ps.SOUP_KEY) for name, tape in tapes.items()}
    return boards, tapes, rates, model


# ---- hand-built 4x4 boards that force the orderings of one step --------------------------------------------------------
def hand_built():
    """(boards int8 [4, 6, 6], tape int8 [1, 4, 2], rates float64 [4, 2], expected steps, winner, final codes), one step:
    0  player 1 RIGHT from (2, 1) without sliding, player 2 UP from (3, 2) sliding: its slide tile lands on player 1's new
       cell (2, 2), player 1 dies on it, player 2 wins from (1, 2); +10 shows on (2, 2)
    1  both slide: player 1's tile fills (2, 2), player 2's target, so player 2 consumes nothing and dies on it; -10 on top
    2  both slide onto the border and die there: a draw
    3  player 1 slides onto player 2's trail and dies; player 2 steps UP without sliding and wins
    (row, column) in the padded 6x6 image."""
    UP, RIGHT, LEFT = 0, 1, 3
    fresh = np.ones((6, 6), np.int8)
    fresh[0], fresh[-1], fresh[:, 0], fresh[:, -1] = -1, -1, -1, -1
    boards, final = np.stack([fresh] * 4), np.stack([fresh] * 4)
    boards[0, 2, 1], boards[0, 3, 2] = 10, -10
    final[0, 2, 1], final[0, 3, 2], final[0, 2, 2], final[0, 1, 2] = -2, -3, 10, -10
    boards[1, 2, 1], boards[1, 3, 2] = 10, -10
    final[1, 2, 1], final[1, 3, 2], final[1, 2, 2], final[1, 2, 3] = -2, -3, -10, 10
    boards[2, 2, 3], boards[2, 3, 2] = 10, -10
    final[2, 2, 3], final[2, 2, 4], final[2, 2, 5] = -2, -2, 10
    final[2, 3, 2], final[2, 3, 1], final[2, 3, 0] = -3, -3, -10
    boards[3, 2, 1], boards[3, 2, 3], boards[3, 4, 4] = 10, -3, -10
    final[3, 2, 1], final[3, 2, 2], final[3, 2, 3], final[3, 4, 4], final[3, 3, 4] = -2, -2, 10, -3, -10
    tape = np.array([[[RIGHT, UP], [RIGHT, UP], [RIGHT, LEFT], [RIGHT, UP]]], np.int8)
    rates = np.array([[-1, 1], [1, 1], [1, 1], [1, -1]], np.float64)
    return boards, tape, rates, np.ones(4, np.int32), np.array([2, 1, 0, 2], np.int8), final


# ---- the recorded sliding episodes ---------------------------------------------------------------------------------------
def recorded_rates(g):
    """float64 [episodes, 2]: what each player's uniform met in the recorded mode."""
    if str(g["mode"]) == "ice":
        return np.repeat(g["slide"].astype(np.float64)[:, None], 2, 1)
    return np.array([[oracle.get_rate(d, w) for w in ws] for d, ws in zip(g["degree"], g["weight"])], np.float64)


def suffixes(g):
    """playout_support.suffixes with the recorded uniforms and rates: (boards, tape, uniforms float32 [K, m, 2], rates
    float64 [m, 2], length, winner, final).  Past an episode's end the uniforms go on at random, like the actions."""
    boards, tape, length, winner, final = ps.suffixes(g)
    off = g["ep_off"].astype(np.int64)
    rows = np.array([t for e in range(len(off) - 1) for t in range(off[e], off[e + 1] - 1)])
    eps = np.searchsorted(off, rows, side="right") - 1
    u = np.random.RandomState(79).random_sample(tape.shape).astype(np.float32)
    for j, t in enumerate(rows):
        u[:length[j], j] = g["uniforms"][t + 1:t + 1 + length[j]]
    return boards, tape, u, recorded_rates(g)[eps], length, winner, final


def starts(g):
    """playout_support.starts with the recorded uniforms and rates."""
    boards, tape, length, winner, final = ps.starts(g)
    off = g["ep_off"].astype(np.int64)
    u = np.random.RandomState(80).random_sample(tape.shape).astype(np.float32)
    for e in range(len(length)):
        u[:length[e], e] = g["uniforms"][off[e]:off[e + 1]]
    return boards, tape, u, recorded_rates(g), length, winner, final
