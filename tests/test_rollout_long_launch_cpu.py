"""The oracle alone on the cases of tests/test_gpu_rollout_long_launch.py (same seeds, same shapes, same sequences): the
conditions that file relies on are counted here and each must be non-zero, so that "the long launch equals the oracle"
means the long launch went through them.  No GPU result enters.

* restarts exactly in steps 63, 64 and 65 of a launch: the old launch boundary, crossed with the ring in every state;
* envs with more than 16, more than 64 and more than 255 restarts inside one launch (side 4): the 16-slot start ring wraps
  dozens of times, nres / hi / the published counts run far past a byte;
* an env that does not restart for 64 consecutive steps of a launch (side 30): the helper tops up nothing for it block
  after block and its ordinal 1 must still be in the ring.  The non-reversing policy gives none: not with this seed (its
  longest run is printed) and with no other that was tried on the CPU — 1 600 seeds of 257 envs x 1 024 steps, 430 M
  env-steps, the longest run of a seed 35 to 48 steps.  The envs come from rollout_long_support.survive_tape, a tape of
  moves that avoid the walls and the trails, played by the tape kernel (case idle-30-*), and the count is asserted there;
* wins and draws per env between two flushes of the byte tallies, and their maxima: the bytes are exercised (a lane holds
  more than one ending of each kind at a flush) and do not wrap (steps at most 128, every count below 256);
* restarts in the last step of a 1 024-step launch and in step 0 of the launch behind it (a call of 1 025 and of 1 032
  steps: the second launch enters by the hand-off of a launch of the cap).
"""
import numpy as np
import pytest

import oracle
from rollout_long_support import CAP, CASES, FLUSH, launch_lengths, longest_idle, model_case, tally_windows

NAMES = ("steps-320-24", "steps-1024-4", "steps-1025-24", "steps-1032-4", "steps-1032-30", "idle-30-257")


@pytest.fixture(scope="module")
def models():
    return {name: model_case(oracle, name) for name in NAMES}


def test_launches_are_the_whole_call_up_to_the_cap(models):
    assert launch_lengths(320) == [320] and launch_lengths(CAP) == [CAP] and launch_lengths(1025) == [CAP, 1] and launch_lengths(1032) == [CAP, 8]
    assert launch_lengths(2 * CAP + 5) == [CAP, CAP, 5] and launch_lengths(130, 64) == [64, 64, 2]
    assert [l["k"] for l in models["steps-320-24"].launches] == [320] * 4
    assert [l["k"] for l in models["steps-1032-4"].launches] == [CAP, 8] * 4
    assert [l["handed"] for l in models["steps-1025-24"].launches] == [False] + [True] * 7
    assert all(name in CASES for name in NAMES)


@pytest.mark.parametrize("name", ("steps-320-24", "steps-1032-4", "steps-1032-30"))
def test_restarts_in_the_steps_around_the_old_boundary(models, name):
    for lch in models[name].launches:
        if lch["k"] > 65:
            for s in (63, 64, 65):
                n = int(lch["hit"][s].sum())
                print(f"{name}: launch of {lch['k']} steps, restarts in step {s}: {n}")
                assert n > 0, (name, s)


def test_many_restarts_inside_one_launch(models):
    seen = {16: 0, 64: 0, 255: 0}
    for name in ("steps-1024-4", "steps-1032-4"):
        for lch in models[name].launches:
            per_env = lch["hit"].sum(0)
            for k in seen:
                seen[k] += int((per_env > k).sum())
    print("env-launches at side 4 with more than 16 / 64 / 255 restarts:", seen)
    assert all(v > 0 for v in seen.values()), seen


def test_an_env_idle_for_64_steps(models):
    nonrev = max(int(longest_idle(lch["hit"]).max()) for lch in models["steps-1032-30"].launches[6:7])
    print("side 30, non-reversing policy, 257 envs x 1 024 steps: the longest run of steps without a restart:", nonrev)
    lch = models["idle-30-257"].launches[0]
    run = longest_idle(lch["hit"])
    print(f"side 30, survive_tape, 257 envs x {lch['k']} steps: envs with 64 and more consecutive steps without a restart: "
          f"{int((run >= 64).sum())}, with none in the whole launch: {int((run == lch['k']).sum())}; the longest run: {int(run.max())}")
    assert lch["k"] == 200 and (run >= 64).sum() > 0
    assert lch["hit"].any(1).sum() > 0                           # and others do restart beside them


@pytest.mark.parametrize("name", NAMES)
def test_byte_tallies_between_two_flushes(models, name):
    hi = np.zeros(4, np.int64)
    several = np.zeros(4, np.int64)
    for lch in models[name].launches:
        w = tally_windows(lch)                                   # [windows, 4, N]
        assert len(w) == (lch["k"] + FLUSH - 1) // FLUSH
        hi = np.maximum(hi, w.max((0, 2)))
        several += (w > 1).sum((0, 2))
    print(f"{name}: per env and flush window, maxima of steps / p1 wins / p2 wins / draws: {hi.tolist()}; windows with more than one: {several.tolist()}")
    assert hi[0] == FLUSH and (hi[1:] > 1).all() and (hi < 256).all(), hi
    assert (hi[1:].sum() <= FLUSH) and (several > 0).all()


@pytest.mark.parametrize("name", ("steps-1025-24", "steps-1032-4", "steps-1032-30"))
def test_restarts_at_the_seam_of_two_launches(models, name):
    seams = 0
    ls = models[name].launches
    for a, b in zip(ls[:-1], ls[1:]):
        if a["k"] == CAP and b["handed"] and b["k"] < CAP:       # the two launches of one call
            last, first = int(a["hit"][CAP - 1].sum()), int(b["hit"][0].sum())
            print(f"{name}: restarts in step {CAP - 1} of a launch of the cap: {last}; in step 0 of the launch behind it: {first}")
            assert last > 0 and first > 0
            seams += 1
    assert seams == 4
