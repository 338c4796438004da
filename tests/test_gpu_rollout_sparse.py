"""Sparse plane stores of the persistent rollout (k_obs_roll): a step stores only the chunks its move wrote and the chunks
where a restarted board differs from the board before, trusting that memory already holds the rest.  These cases check
what such a store could get wrong: a buffer changed between rollouts by every writer the API offers, episodes that end
on the border (a head overwrites a WALL cell) or head-on on one cell and the restarts that follow them, sizes around the
residency limits and ragged last tiles.  Every byte of env.obs, grid() and state() is compared with the CPU oracle
driven the same way.  No tolerances anywhere."""
import numpy as np
import pytest

from rollout_support import Ref, check_against_oracle, gpu_modules, np_, pull, restore_threads, start_positions

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

@pytest.fixture(scope="module")
def T():
    return gpu_modules()


def check(env, ref, tag):
    """Every byte a caller can read back against the oracle."""
    check_against_oracle(pull(env), ref, tag, totals=False)


def rollout(env, ref, K, nonrev):
    env.rollout_random(K, nonreversing=nonrev)
    for _ in range(K):
        ref.step(nonrev=nonrev)


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N,W", [(1, 10), (63, 24), (65, 24), (1000, 24), (1000, 32), (4096, 10)])
def test_hand_off_through_every_writer(T, N, W, nonrev):
    """Between rollouts the buffer is changed by tron_reset (env_mask + explicit start_pos), a step with the caller's
    actions, steps through TRON_STEP_INCREMENTAL and tron_set_weight_degree; each rollout must find in memory exactly
    what its stores skip."""
    tv, oracle = T
    env = tv.VecTron(N, W, seed=41, rank=6, obs_format="codes")
    assert env.obs_is_state
    ref = Ref(oracle, N, W, seed=41, rank=6)
    env.reset()
    rs = np.random.RandomState(N * 100 + W + int(nonrev))
    rollout(env, ref, 20, nonrev)
    check(env, ref, "first rollout")

    m = (rs.rand(N) < 0.3).astype(np.int8)
    m[0] = 1
    sp = start_positions(rs, N, W)
    env.reset(mask=torch.from_numpy(m), start_pos=torch.from_numpy(sp))
    ref.v.set_starts(sp, mask=m)
    check(env, ref, "tron_reset with env_mask and start_pos")
    rollout(env, ref, 65, nonrev)
    check(env, ref, "rollout after tron_reset")

    acts = rs.randint(0, 4, (N, 2)).astype(np.int8)
    _, reward, done, winner = env.step(torch.from_numpy(acts))
    d, w, r = ref.step(acts)
    assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
    check(env, ref, "step with the caller's actions")
    rollout(env, ref, 2, nonrev)
    check(env, ref, "rollout after a step with actions")

    env.incremental = True
    for _ in range(3):
        env.step(nonreversing=nonrev)
        ref.step(nonrev=nonrev)
    env.incremental = False
    check(env, ref, "incremental steps")
    rollout(env, ref, 64, nonrev)
    check(env, ref, "rollout after incremental steps")

    wt = rs.randint(40, 102, (N, 2)).astype(np.int16)
    dg = rs.randint(-30, 31, N).astype(np.int16)
    env.set_weight_degree(torch.from_numpy(wt), torch.from_numpy(dg))
    ref.v.weight[:] = wt
    ref.v.degree[:] = dg
    check(env, ref, "tron_set_weight_degree")
    for K in (1, 2, 64, 65):
        rollout(env, ref, K, nonrev)
        check(env, ref, f"rollout of {K} after tron_set_weight_degree")


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N,W,seed", [(1000, 10, 3), (1000, 24, 8), (999, 32, 12)])
def test_border_deaths_and_same_cell_draws(T, N, W, seed, nonrev):
    """Episodes that end with a head on the border (it overwrites a WALL cell, which the restart must put back) and
    head-on draws on one cell (P2's head over P1's), then the restarts that follow: the oracle must show at least one of
    each in every rollout of the seed, and the GPU must match it byte for byte after every rollout and on through the
    next restarts (per-step launches)."""
    tv, oracle = T
    env = tv.VecTron(N, W, seed=seed, rank=1, obs_format="codes")
    ref = Ref(oracle, N, W, seed=seed, rank=1, events=True)    # (looks at the finished boards before they restart)
    env.reset()
    for K in (20, 65, 64):
        b0, s0 = ref.border_deaths, ref.same_cell
        rollout(env, ref, K, nonrev)
        print(f"rollout of {K}: {ref.border_deaths - b0} border deaths, {ref.same_cell - s0} same-cell draws")
        assert ref.border_deaths > b0 and ref.same_cell > s0, "the seed must show both kinds of ending"
        check(env, ref, f"rollout of {K}")
    for k in range(6):
        env.step(nonreversing=nonrev)
        ref.step(nonrev=nonrev)
        check(env, ref, f"per-step launch {k} after the rollouts")


# the whole 65 536 x 24x24 batch, twice that (more than one round of workgroups), W = 10 and 32, ragged last tiles
SIZES = [(1, 24), (63, 24), (65, 24), (1000, 24), (1000, 10), (1000, 32), (4096, 10), (4096, 32), (65536, 24),
         (131072, 24)]


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N,W", SIZES)
def test_sizes_around_residency_limits(T, N, W, nonrev):
    """A launch of 64 steps and one of 6, then per-step launches through the next restarts."""
    tv, oracle = T
    big = N >= 65536
    if big:
        gpu_modules(threads=True)
    try:
        env = tv.VecTron(N, W, seed=29, rank=2, obs_format="codes")
        ref = Ref(oracle, N, W, seed=29, rank=2)
        env.reset()
        rollout(env, ref, 70, nonrev)
        check(env, ref, "rollout of 70")
        for k in range(2 if big else 8):
            env.step(nonreversing=nonrev)
            ref.step(nonrev=nonrev)
        check(env, ref, "per-step launches after the rollout")
    finally:
        restore_threads(oracle)
