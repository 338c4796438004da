"""The store list of the persistent rollout (k_obs_roll): a step's chunk stores go through a wave-wide list in LDS, so a lane
stores chunks of other lanes' envs and, after a restart, writes other lanes' boards.  What that can get wrong: the prefix sum
over ragged waves, a list longer than one trip (every env of a wave restarting at once), the list's last entries, the full
64-bit mask at W = 30 (64 chunks per board, the shift by 63), the short last chunk at W = 4, a board rebuilt by another lane
and read by its own lane's next move, waves with nothing to store.

Every byte of env.obs, grid() and state() and the totals are compared with the CPU oracle, no tolerances.  Rollouts are
interleaved with single step() calls, whose done / winner / reward arrays are compared as well (tron_rollout_random returns
totals only).

A wave with an empty list whose envs are all finished cannot be made through the API: tron_rollout_random always sets autoreset,
so a finished env restarts (and stores) in the launch's first step.  The empty list that can occur is that of a wave without
envs, in a ragged last workgroup of four waves: test_four_wave_workgroups."""
import numpy as np
import pytest

from rollout_support import Ref, check_against_oracle, gpu_modules, new_totals, np_, pull, restore_threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def T():
    return gpu_modules()


def check(env, ref, tag):
    """Every byte a caller can read back against the oracle."""
    check_against_oracle(pull(env), ref, tag, totals=False)


def rollout(env, ref, K, nonrev, tag=""):
    totals = new_totals()
    env.rollout_random(K, totals, nonreversing=nonrev)
    before = ref.totals.copy()
    for _ in range(K):
        ref.step(nonrev=nonrev)
    check(env, ref, f"rollout of {K} {tag}")
    assert np.array_equal(np_(totals), ref.totals - before), f"totals of the rollout of {K} {tag}"


def single_step(env, ref, nonrev, tag=""):
    _, reward, done, winner = env.step(nonreversing=nonrev)
    d, w, r = ref.step(nonrev=nonrev)
    assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r), f"step {tag}"


def make(T, N, W, seed, rank):
    tv, oracle = T
    env = tv.VecTron(N, W, seed=seed, rank=rank, obs_format="codes")
    assert env.obs_is_state
    env.reset()
    return env, Ref(oracle, N, W, seed, rank)


# W = 4: 3 chunks, the last one short (36 = 2 x 16 + 4); 6: 4 chunks, no short one; 24: the benchmark's; 30: 64 chunks.
# N: one lane; a wave less / exactly / plus one env; 257 and 1 000: several one-wave workgroups and a ragged last wave.
@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W", [4, 6, 24, 30])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_rollouts_and_steps(T, N, W, nonrev):
    """K = 1, 2, 7 and 64 on the same env, a step() with its records after each: every launch starts from what the one before
    left in memory, and every step() reads boards the rollout left.  K = 1 is a single per-step launch (the host sends only
    k_steps > 1 to the persistent kernel), so it does not run the list: it checks the seam between the two paths."""
    env, ref = make(T, N, W, seed=100 + N + W, rank=3)
    for K in (1, 2, 7, 64):
        rollout(env, ref, K, nonrev, tag=f"N {N} W {W}")
        single_step(env, ref, nonrev, tag=f"after the rollout of {K}")
    check(env, ref, "after the last step")
    if N >= 63:
        assert max(ref.restarts_per_step) > 0, "at least one restart must have gone through the list"


@pytest.mark.parametrize("W,N", [(4, 64), (4, 200), (6, 64), (24, 64)])
def test_every_env_of_a_wave_restarts_at_once(T, W, N):
    """Steps without autoreset until every env has finished; the persistent launch's first step then restarts all 64 envs of a wave
    at once, each with its whole episode's chunks and the two new heads: the list is as full as the API can make it and takes
    more than one trip (64 envs x at least 2 chunks)."""
    env, ref = make(T, N, W, seed=9, rank=1)
    rollout(env, ref, 2, False)
    for _ in range(400):
        if (ref.v.done == 1).all():
            break
        _, reward, done, winner = env.step(autoreset=False)
        _, d, w, r = ref.v.step(None, autoreset=False, want_obs=False)
        assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
    assert (ref.v.done == 1).all(), "every env must have finished before the rollout"
    check(env, ref, "all envs finished")
    ref.restarts_per_step.clear()
    rollout(env, ref, 2, False, tag="restarting every env")      # (two steps: one alone would be a per-step launch)
    assert ref.restarts_per_step[0] == N
    single_step(env, ref, False)
    rollout(env, ref, 64, False, tag="after the full restart")
    single_step(env, ref, False)


# Above 64 envs x the number of CUs a workgroup is four waves, each with a list of its own (at 30x30 three: four do not
# fit the LDS).  + 1: one lane of wave 0 and three waves without envs (empty lists); + 200: three full waves and 8 lanes.
@pytest.mark.parametrize("N,W,Ks", [(16384 + 1, 6, (7, 2)), (16384 + 200, 6, (3,)), (16384 + 65, 30, (2,))])
def test_four_wave_workgroups(T, N, W, Ks):
    _, oracle = gpu_modules(threads=True)
    try:
        env, ref = make(T, N, W, seed=N % 1000, rank=2)
        for K in Ks:
            rollout(env, ref, K, False, tag=f"N {N} W {W}")
            single_step(env, ref, False)
    finally:
        restore_threads(oracle)
