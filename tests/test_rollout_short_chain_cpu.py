"""On the oracle alone: the inputs of tests/test_gpu_rollout_short_chain.py (same seed, stream, shapes and sequence of
calls) contain the cases the shorter step chain can break, each at least once at every side it can occur at:

  an env with 0, with exactly 1 and with 2 or more restarts in a launch (the epilogue's rs4.nstart conversion, which only
  a lane that restarted makes, and the envp rule); a restart in a launch's last step (eplen 0 at the epilogue) and in the first
  step behind a hand-off (a ring slot written by the launch before, read in cell space); both start heads in one chunk
  and in one dword (the restart's chunk writes in front of its two nibble writes); a first move that leaves the start
  chunk (the move marks the new chunks only); a dead head on each border and on the short last chunk; a head in chunk
  63 at side 30; a lane that enters a launch finished (one move fewer than steps).

The counts are printed; the smallest are recorded in profiles/r31_rollout_ab.txt.
"""
import pytest

from rollout_short_chain_support import COUNTS, OPS, SIDES, Model, host_tape

N = 257


@pytest.fixture(scope="module")
def oracle():
    import oracle
    return oracle


def count(oracle, W, fair, kind):
    mod = Model(oracle, N, W, fair, kind)
    for i, op in enumerate(OPS):
        tape = host_tape(N, op[1], salt=i) if op[0] == "call" and kind in ("tape", "records") else None
        mod.op(op, tape)
    return mod


@pytest.mark.parametrize("kind", ["uniform", "nonreversing", "tape"])   # (records plays the tape kind's actions)
@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("W", SIDES)
def test_inputs_contain_the_cases(oracle, W, fair, kind):
    mod = count(oracle, W, fair, kind)
    for k in COUNTS:
        print(f"side {W}, {N} envs, fair {fair}, {kind}: {k} {mod.c[k]}")
    for k in COUNTS:
        if mod.can_occur(k):
            assert mod.c[k] >= 1, (W, fair, kind, k)
        else:
            assert mod.c[k] == 0, (W, fair, kind, k)
