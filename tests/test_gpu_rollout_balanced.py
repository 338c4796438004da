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
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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
    """The oracle with autoreset done by hand: per-step records as a step with autoreset reports them, and the totals."""

    def __init__(self, oracle, N, W, seed, rank):
        self.oracle = oracle
        self.v = oracle.VecOracle(N, W, seed=seed, stream=rank)
        self.v.reset_all()
        self.totals = np.zeros(4, np.int64)
        self.restarts = []                    # per step: how many envs restarted

    def step(self, nonrev=False):
        v = self.v
        stepped = v.done == 0                 # an env that was finished before the step is not stepped, only restarted
        _, d, w, r = v.step(None, autoreset=False, want_obs=False, nonreversing=nonrev)
        d, w, r = d.copy(), w.copy(), r.copy()
        fin = (d == 1) & stepped
        self.totals += np.array([stepped.sum(), (fin & (w == 1)).sum(), (fin & (w == 2)).sum(), (fin & (w == 0)).sum()], np.int64)
        self.restarts.append(int((d == 1).sum()))
        if (d == 1).any():
            v.reset_masked(d == 1)
        return d, w, r

    def obs(self):
        g = self.v.grid
        return np.stack([self.oracle.state_for_player(g, 1), self.oracle.state_for_player(g, 2)], 1)


def check(env, ref, tag):
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
    assert np.array_equal(c[:, 0], v.tick) and np.array_equal(c[:, 1], v.episode) and np.array_equal(c[:, 2], v.eplen), tag


def rollout(env, ref, K, nonrev, tag=""):
    totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    env.rollout_random(K, totals, nonreversing=nonrev)
    before = ref.totals.copy()
    for _ in range(K):
        ref.step(nonrev)
    check(env, ref, f"rollout of {K} {tag}")
    assert np.array_equal(np_(totals), ref.totals - before), f"totals of the rollout of {K} {tag}"


def single_step(env, ref, nonrev, tag=""):
    _, reward, done, winner = env.step(nonreversing=nonrev)
    d, w, r = ref.step(nonrev)
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
        assert max(ref.restarts) > 0, "at least one restart must have gone through the list"


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
    ref.restarts.clear()
    rollout(env, ref, 2, False, tag="restarting every env")      # (two steps: one alone would be a per-step launch)
    assert ref.restarts[0] == N
    single_step(env, ref, False)
    rollout(env, ref, 64, False, tag="after the full restart")
    single_step(env, ref, False)


# Above 64 envs x the number of CUs a workgroup is four waves, each with a list of its own (at 30x30 three: four do not
# fit the LDS).  + 1: one lane of wave 0 and three waves without envs (empty lists); + 200: three full waves and 8 lanes.
@pytest.mark.parametrize("N,W,Ks", [(16384 + 1, 6, (7, 2)), (16384 + 200, 6, (3,)), (16384 + 65, 30, (2,))])
def test_four_wave_workgroups(T, N, W, Ks):
    _, oracle = T
    oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
    try:
        env, ref = make(T, N, W, seed=N % 1000, rank=2)
        for K in Ks:
            rollout(env, ref, K, False, tag=f"N {N} W {W}")
            single_step(env, ref, False)
    finally:
        oracle.set_threads(1)
