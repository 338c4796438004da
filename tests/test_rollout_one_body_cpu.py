"""On the oracle alone: the inputs of tests/test_gpu_rollout_one_body.py (same seed, stream, shapes and sequence of calls)
contain the cases the one step body of the roll_resident family can break, each at least once at every side it can occur at.

A restart is due in the step its game finishes in (the lane has made its move and skipped the move's board work) and, for an
env that entered the launch finished, in the launch's first step without a move; the body then does the move's board work
at the start cells.  The cases, with the smallest count over sides x fair x {uniform, non-reversing, tape} at 257 envs (each
taken over the sides it can occur at):

  a restart whose start cell lies in a chunk of the finished game's trail (refreshed by the restart and stale by the mask
  at once) 5 472; both start cells in one chunk 8 and in one dword 8 (side 30); a move whose new head lands in a stale
  chunk in the step right after the env's restart 6 110; both new heads in one stale chunk 22; a game that ends in its
  first move right after a restart, so that the start word read at that restart is used in the very next step 950; a
  restart in a launch's last step 945 and in the first step behind a hand-off 529; an env that enters a launch finished
  and restarts there without a move 88; a finishing move whose head dies on the border wall up / down / left / right
  1 609 / 1 591 / 1 596 / 1 610, on the short last chunk 180 (sides 4 and 24), in chunk 63 at side 30 764.
  At 65 envs: a step in which all 64 lanes of the first wave move and none restarts, 1 in every group — the first row of
  the safe tape (rollout_one_body_support.safe_tape; random play has none: a third of the env-steps are restarts).  At 1
  env (a wave of one lane): steps in which the env moves and does not restart 204 at the least, steps in which it restarts 72.

Three cases of the issue's list cannot occur at any side, and the test asserts that they do not: a start cell on the short
last chunk or in chunk 63 (those chunks are cells of the border's last row; a dead head lands there, counted above), and an
env that enters a launch finished behind a hand-off (the hand-off is taken behind a launch with autoreset alone, which leaves
no env finished; entered-finished envs come behind per-step steps without autoreset, counted above).

The counts are printed.
"""
import pytest

from rollout_one_body_support import COUNTS, OPS, SIDES, Model, host_tape, safe_tape

WAVE_CASES = ("step_all_move_none_restarts", "step_every_env_restarts", "restart_without_move")


@pytest.fixture(scope="module")
def oracle():
    import oracle
    return oracle


def count(oracle, N, W, fair, kind):
    mod = Model(oracle, N, W, fair, kind)
    for i, op in enumerate(OPS):
        tape = host_tape(N, op[1], salt=i) if op[0] == "call" and kind in ("tape", "records") else None
        if op[0] == "safe":
            tape = safe_tape(mod.ref.v.pos, W, op[1], salt=i)
        mod.op(op, tape)
    return mod


@pytest.mark.parametrize("kind", ["uniform", "nonreversing", "tape"])   # (records plays the tape kind's actions)
@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("W", SIDES)
def test_inputs_contain_the_cases(oracle, W, fair, kind):
    mod = count(oracle, 257, W, fair, kind)
    for k in COUNTS:
        print(f"side {W}, 257 envs, fair {fair}, {kind}: {k} {mod.c[k]}")
    for k in COUNTS:
        if k in ("step_all_move_none_restarts", "step_every_env_restarts"):
            continue                                                 # (asked of the one-env wave below)
        if mod.can_occur(k):
            assert mod.c[k] >= 1, (W, fair, kind, k)
        else:
            assert mod.c[k] == 0, (W, fair, kind, k)


@pytest.mark.parametrize("kind", ["uniform", "nonreversing", "tape"])
@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("W", SIDES)
def test_whole_wave_steps(oracle, W, fair, kind):
    """65 envs: a step in which all 64 lanes of the first wave move and none restarts (the safe tape's first row; random play
    has none).  1 env, a wave of one lane: steps in which the env moves and does not restart, and steps in which it restarts."""
    m65, m1 = count(oracle, 65, W, fair, kind), count(oracle, 1, W, fair, kind)
    for k in WAVE_CASES:
        print(f"side {W}, fair {fair}, {kind}: {k} 65 envs {m65.c[k]}, 1 env {m1.c[k]}")
    assert m65.c["step_all_move_none_restarts"] >= 1, (W, fair, kind)
    assert m1.c["step_every_env_restarts"] >= 1, (W, fair, kind)
    assert m1.c["step_all_move_none_restarts"] >= 1, (W, fair, kind)
