"""Sparse plane stores of the persistent rollout (k_obs_roll): a step stores only the chunks its move wrote and the chunks
where a restarted board differs from the board before, trusting that memory already holds the rest.  These cases check
what such a store could get wrong: a buffer changed between rollouts by every writer the API offers, episodes that end
on the border (a head overwrites a WALL cell) or head-on on one cell and the restarts that follow them, sizes around the
residency limits and ragged last tiles.  Every byte of env.obs, grid() and state() is compared with the CPU oracle
driven the same way.  No tolerances anywhere."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree", "counters")
WALL, P1_HEAD = -1, 2          # raw tile values (map.py:9-17)


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tron.vec as tv
    import oracle
    return tv, oracle


def np_(t):
    return t.detach().cpu().numpy()


class Ref:
    """The oracle with autoreset done by hand (a step without autoreset, then a reset of the envs that finished: what
    orc_vec_step does with autoreset), so that the boards that finished can be looked at before they restart."""

    def __init__(self, oracle, N, W, seed, rank):
        self.oracle = oracle
        self.v = oracle.VecOracle(N, W, seed=seed, stream=rank)
        self.v.reset_all()
        S = W + 2
        b = np.zeros((S, S), bool)
        b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
        self.border = b.reshape(-1)
        self.border_deaths = 0          # episodes that ended with a head on a border cell
        self.same_cell = 0              # episodes that ended with both heads on one cell (P2's head over P1's)

    def step(self, actions=None, nonrev=False, count=False):
        v = self.v
        if not count:
            _, d, w, r = v.step(actions, autoreset=True, want_obs=False, nonreversing=nonrev)
            return d, w, r
        _, d, w, r = v.step(actions, autoreset=False, want_obs=False, nonreversing=nonrev)
        fin = d == 1                     # (every env was live before the step: autoreset)
        if fin.any():
            g = v.grid[fin]
            self.border_deaths += int((g[:, self.border] != WALL).any(1).sum())
            self.same_cell += int((~(g == P1_HEAD).any(1)).sum())
            v.reset_masked(fin)
        return d, w, r

    def obs(self):
        g = self.v.grid
        return np.stack([self.oracle.state_for_player(g, 1), self.oracle.state_for_player(g, 2)], 1)


def check(env, ref, tag):
    """Every byte a caller can read back against the oracle."""
    v, N = ref.v, ref.v.N
    torch.cuda.synchronize()
    st = env.state()
    assert np.array_equal(np_(env.obs).reshape(N, 2, -1), ref.obs()), tag
    assert np.array_equal(np_(env.grid()).reshape(N, -1), v.grid), tag
    assert np.array_equal(np_(st["pos"]), v.pos) and np.array_equal(np_(st["alive"]), v.alive), tag
    assert np.array_equal(np_(st["dir"]), v.dir), tag
    assert np.array_equal(np_(st["done"]), v.done) and np.array_equal(np_(st["winner"]), v.winner), tag
    assert np.array_equal(np_(st["weight"]), v.weight) and np.array_equal(np_(st["degree"]), v.degree), tag
    c = np_(st["counters"]).astype(np.uint32)
    assert np.array_equal(c[:, 0], v.tick) and np.array_equal(c[:, 1], v.episode), tag
    assert np.array_equal(c[:, 2], v.eplen), tag


def rollout(env, ref, K, nonrev, count=False):
    env.rollout_random(K, nonreversing=nonrev)
    for _ in range(K):
        ref.step(nonrev=nonrev, count=count)


def start_positions(rs, N, W):
    sp = rs.randint(0, W, (N, 4)).astype(np.int8)
    clash = (sp[:, 0] == sp[:, 2]) & (sp[:, 1] == sp[:, 3])
    sp[clash, 3] = (sp[clash, 1] + 1) % W
    return sp


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
    ref = Ref(oracle, N, W, seed=seed, rank=1)
    env.reset()
    for K in (20, 65, 64):
        b0, s0 = ref.border_deaths, ref.same_cell
        rollout(env, ref, K, nonrev, count=True)
        print(f"rollout of {K}: {ref.border_deaths - b0} border deaths, {ref.same_cell - s0} same-cell draws")
        assert ref.border_deaths > b0 and ref.same_cell > s0, "the seed must show both kinds of ending"
        check(env, ref, f"rollout of {K}")
    for k in range(6):
        env.step(nonreversing=nonrev)
        ref.step(nonrev=nonrev, count=True)
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
        oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
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
        oracle.set_threads(1)
