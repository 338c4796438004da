"""What the tron_playout_values tests share (tests/test_playout_values_model_cpu.py, tests/test_gpu_playout_values.py): the
host model — tron_playout_values is defined through tron_playout_codes, so its model is a composition of
playout_support.playout, which is pinned to the recorded episodes — the maximin in numpy, and the boards both files use.
A plain module, imported by name; nothing here needs a GPU."""
import numpy as np

import playout_support as ps

WIDTHS = (4, 5, 10, 32)
COPIES = (1, 3, 4, 5)
# 38 of the soup's 1 061 boards: every 31st, and one of each kind of rejected board (no +10, two +10, a +10 on the border)
SELECT = tuple(sorted(set(range(0, ps.SOUP_N, 31)) | {5, 58, 111}))
REJECTED = (5, 58, 111)
KEY = dict(seed=0xFACADE, stream_id=9, call=(3 << 32) | 11)


def ks(W):
    return (0, 1, 7, W * W)


def fan_out(codes, k_steps, copies):
    """The launch tron_playout_values stands for: (boards [n * 16 * copies, S, S], tape int8 [k_steps, n * 16 * copies, 2]).
    Index q = ((i * 16 + a1 * 4 + a2) * copies + j) holds board i; the tape's row 0 holds (a1, a2), every other row is
    negative (safe draws)."""
    codes = np.ascontiguousarray(codes, np.int8)
    n = len(codes)
    boards = np.repeat(codes, 16 * copies, axis=0)
    tape = np.full((k_steps, n * 16 * copies, 2), -1, np.int8)
    if k_steps:
        move = (np.arange(n * 16 * copies) // copies) % 16
        tape[0, :, 0], tape[0, :, 1] = move >> 2, move & 3
    return boards, tape


def tally(steps, winner, n, copies):
    """(counts int32 [n, 4, 4, 4], steps int32 [n, 4, 4]) of one fanned-out launch's out_steps and out_winner."""
    q = np.arange(n * 16 * copies)
    board, move = q // (16 * copies), (q // copies) % 16
    counts = np.zeros((n, 4, 4, 4), np.int32)
    total = np.zeros((n, 4, 4), np.int32)
    played = winner != -2
    np.add.at(counts, (board[played], move[played] >> 2, move[played] & 3, winner[played].astype(np.int64) & 3), 1)   # -1 -> 3
    np.add.at(total, (board, move >> 2, move & 3), steps)              # a rejected board's steps are 0
    return counts, total


def pick(counts):
    """int8 [n, 2]: each player's maximin move on m = wins of 1 - wins of 2 (negated for player 2): the first move in UP,
    RIGHT, DOWN, LEFT order whose worst case over the opponent's four moves is greatest; -1 where nothing was played."""
    counts = np.asarray(counts).astype(np.int64)
    m = counts[..., 1] - counts[..., 2]                                # [n, a1, a2]
    act = np.stack([m.min(2).argmax(1), (-m).min(1).argmax(1)], 1).astype(np.int8)
    act[counts.reshape(len(counts), -1).sum(1) == 0] = -1
    return act


def values_model(codes, k_steps, copies, ks=None, **key):
    """The model of one tron_playout_values call: (counts, steps, actions); with `ks` {k: that triple} at several k_steps
    at once (a playout's first k steps do not depend on how many follow)."""
    many = sorted(set([k_steps] if ks is None else ks))
    n = len(codes)
    boards, tape = fan_out(codes, many[-1], copies)
    out = {}
    for k, ((steps, winner, _), _) in ps.playout(boards, tape, ks=many, **key).items():
        counts, total = tally(steps, winner, n, copies)
        out[k] = (counts, total, pick(counts))
    return out if ks is not None else out[k_steps]


_cache = {}


def boards(W):
    """The selected boards of width W, [38, S, S]."""
    return ps.soup(W)[0][list(SELECT)]


def model(W, copies, **change):
    """{k: (counts, steps, actions)} of boards(W) at ks(W) under KEY (with `change`), computed once per process and never
    changed."""
    at = (W, copies, tuple(sorted(change.items())))
    if at not in _cache:
        _cache[at] = values_model(boards(W), None, copies, ks=ks(W), **dict(KEY, **change))
    return _cache[at]
