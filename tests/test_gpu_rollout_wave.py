"""The persistent rollout with one lane per env (k_obs_roll): a wave steps its own envs with no barrier, the boards sit
in LDS at 4 bits per cell, and the chunks a step stores come from a per-env 64-bit mask instead of a search.  What
that can get wrong: ragged waves and workgroups, the 64-step launch seam, the mask's width limit (cpe = 64 at W = 30;
wider boards must take the walking kernel), masks that grow over long episodes, masks rebuilt by the prologue after
every writer the API has changed the buffer, finished envs found at the start of a launch.

Every byte of env.obs, grid() and state() and the totals are compared with the CPU oracle driven the same way; no
tolerances.  tron_rollout_random implies autoreset and returns totals only, so done / winner / reward are compared
as the totals of every rollout and as the per-step arrays of the step() calls between rollouts; envs that finished
under autoreset=False reach the rollout as finished envs (nothing is redrawn for them before it)."""
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


def tally(d, w, stepped):
    fin = (d == 1) & stepped
    return np.array([int(stepped.sum()), int((fin & (w == 1)).sum()), int((fin & (w == 2)).sum()), int((fin & (w == 0)).sum())],
                    np.int64)


class Ref:
    """The oracle with autoreset done by hand, so that finished boards can be looked at before they restart."""

    def __init__(self, oracle, N, W, seed, rank):
        self.oracle = oracle
        self.v = oracle.VecOracle(N, W, seed=seed, stream=rank)
        self.v.reset_all()
        S = W + 2
        b = np.zeros((S, S), bool)
        b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
        self.border = b.reshape(-1)
        self.border_deaths = self.same_cell = self.long_episodes = 0
        self.totals = np.zeros(4, np.int64)

    def step(self, actions=None, nonrev=False):
        """One step with autoreset; returns done / winner / reward as a step with autoreset reports them."""
        v = self.v
        was_done = v.done == 1               # finished before the step: not stepped, restarted by the autoreset
        _, d, w, r = v.step(actions, autoreset=False, want_obs=False, nonreversing=nonrev)
        d, w, r = d.copy(), w.copy(), r.copy()
        self.totals += tally(d, w, ~was_done)
        fin = d == 1
        if fin.any():
            g = v.grid[fin & ~was_done]
            self.border_deaths += int((g[:, self.border] != WALL).any(1).sum())
            self.same_cell += int((~(g == P1_HEAD).any(1)).sum())
            self.long_episodes += int((v.eplen[fin] >= 20).sum())
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


def rollout(env, ref, K, nonrev=False, tag=""):
    """K steps both ways; the rollout's totals against the oracle's."""
    totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    env.rollout_random(K, totals, nonreversing=nonrev)
    before = ref.totals.copy()
    for _ in range(K):
        ref.step(nonrev=nonrev)
    check(env, ref, f"rollout of {K} {tag}")
    assert np.array_equal(np_(totals), ref.totals - before), f"totals of the rollout of {K} {tag}"


def make(T, N, W, seed, rank):
    tv, oracle = T
    env = tv.VecTron(N, W, seed=seed, rank=rank, obs_format="codes")
    assert env.obs_is_state
    env.reset()
    return env, Ref(oracle, N, W, seed, rank)


# Up to 64 x (number of CUs) envs the host launches one 64-env wave per workgroup, so there wave and workgroup are the same:
# 1: one lane; 63 / 64 / 65: a wave less / more than one env; 200: several waves and a ragged last one
@pytest.mark.parametrize("W", [6, 24])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
def test_ragged_waves_and_launch_seams(T, N, W):
    """k in {1, 3, 64, 65, 130} one after another on the same env: 65 and 130 cross the 64-step launch boundary, and
    every rollout starts from what the one before left in memory."""
    env, ref = make(T, N, W, seed=31 + N, rank=2)
    for K in (1, 3, 64, 65, 130):
        rollout(env, ref, K)


# Above that (16 384 envs on the MI355X's 256 CUs) a workgroup is four waves of 64 envs, the benchmark's shape.  Its last
# workgroup: + 1: one lane of wave 0, three empty waves; + 65: a full wave, one lane, two empty waves;
# + 200: three full waves and 8 lanes of the fourth; + 255: one lane short of a full workgroup
@pytest.mark.parametrize("N", [16384 + 1, 16384 + 65, 16384 + 200, 16384 + 255])
def test_ragged_four_wave_workgroups(T, N):
    """The benchmark's launch shape with a ragged tail, through the 64-step seam (65 = 64 + 1, then 3 from memory)."""
    _, oracle = T
    oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
    try:
        env, ref = make(T, N, 6, seed=N % 1000, rank=2)
        rollout(env, ref, 65)
        rollout(env, ref, 3)
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("W,K", [(30, 65), (32, 65), (9, 20)])
def test_mask_width_limits_and_routing(T, W, K):
    """W = 30: 64 chunks per board, the last mask that fits (bit 63 is the last row's chunk).  W = 32: 73 chunks, the host
    must route to k_obs_roll_walk.  W = 9: an odd side stays on the board-owning layout (k_tile_roll)."""
    tv, oracle = T
    N = 130
    env = tv.VecTron(N, W, seed=5, rank=3, obs_format="codes")
    assert env.obs_is_state == (W % 2 == 0)
    env.reset()
    ref = Ref(oracle, N, W, 5, 3)
    assert ((W + 2) ** 2 + 15) // 16 == {30: 64, 32: 73, 9: 8}[W]
    rollout(env, ref, K)
    rollout(env, ref, 3)


@pytest.mark.parametrize("N,W", [(65, 6), (200, 24)])
def test_nonreversing_and_finished_envs(T, N, W):
    """nonreversing=True, and envs that finished under autoreset=False: they stay finished through further such steps
    (nothing is redrawn), and the rollout that follows finds them finished at its first step and restarts them."""
    env, ref = make(T, N, W, seed=17, rank=1)
    rollout(env, ref, 3, nonrev=True)
    for k in range(4 if W == 6 else 8):             # (oracle, on the CPU: 56 of 65 / 176 of 200 envs have finished by then)
        _, reward, done, winner = env.step(autoreset=False, nonreversing=True)
        _, d, w, r = ref.v.step(None, autoreset=False, want_obs=False, nonreversing=True)
        assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
    assert (ref.v.done == 1).any() and (ref.v.done == 0).any()
    check(env, ref, "steps without autoreset")
    rollout(env, ref, 65, nonrev=True, tag="over finished envs")
    rollout(env, ref, 64, nonrev=True)


# chosen on the CPU with the oracle (N = 200, W = 24, non-reversing, 130 steps) so that all three counts are non-zero
LONG_SEED, LONG_RANK = 7, 1


def test_long_episodes(T):
    """Non-reversing actions on 24x24 for 130 steps: masks grow to many chunks before a restart stores them back."""
    env, ref = make(T, 200, 24, seed=LONG_SEED, rank=LONG_RANK)
    rollout(env, ref, 130, nonrev=True)
    print(f"episodes of >= 20 steps: {ref.long_episodes}, border deaths: {ref.border_deaths}, same-cell: {ref.same_cell}")
    assert ref.long_episodes > 0, "at least one episode must reach 20 steps before restarting"
    assert ref.border_deaths > 0, "at least one episode must end with a head on a border cell"
    assert ref.same_cell > 0, "at least one episode must end with both heads on one cell"


def start_positions(rs, N, W):
    sp = rs.randint(0, W, (N, 4)).astype(np.int8)
    clash = (sp[:, 0] == sp[:, 2]) & (sp[:, 1] == sp[:, 3])
    sp[clash, 3] = (sp[clash, 1] + 1) % W
    return sp


@pytest.mark.parametrize("N,W", [(65, 6), (200, 24)])
def test_writers_between_rollouts(T, N, W):
    """Every writer the API has, each between two rollouts: a masked reset with explicit start positions (the state
    setter), weights and degrees through the reset and through tron_set_weight_degree, steps with the caller's actions
    and steps through TRON_STEP_INCREMENTAL.  The prologue's rebuilt mask must cover what they changed: the rollout
    after each runs through restarts (65 steps) and is compared in full."""
    env, ref = make(T, N, W, seed=43, rank=5)
    rs = np.random.RandomState(N + W)
    rollout(env, ref, 20)

    m = (rs.rand(N) < 0.4).astype(np.int8)
    m[0] = 1
    sp = start_positions(rs, N, W)
    env.reset(mask=torch.from_numpy(m), start_pos=torch.from_numpy(sp))
    ref.v.set_starts(sp, mask=m)
    check(env, ref, "masked reset with start positions")
    rollout(env, ref, 65, tag="after the masked reset")

    wt = rs.randint(40, 102, (N, 2)).astype(np.int16)
    dg = rs.randint(-30, 31, N).astype(np.int16)
    env.set_weight_degree(torch.from_numpy(wt), torch.from_numpy(dg))
    ref.v.weight[:] = wt
    ref.v.degree[:] = dg
    rollout(env, ref, 65, tag="after tron_set_weight_degree")

    for _ in range(5):
        acts = rs.randint(0, 4, (N, 2)).astype(np.int8)
        _, reward, done, winner = env.step(torch.from_numpy(acts))
        d, w, r = ref.step(acts)
        assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
    check(env, ref, "steps with the caller's actions")
    rollout(env, ref, 65, tag="after steps with actions")

    env.incremental = True
    for _ in range(3):
        env.step()
        ref.step()
    env.incremental = False
    check(env, ref, "incremental steps")
    rollout(env, ref, 65, tag="after incremental steps")


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N,W,K", [(200, 24, 130), (65, 30, 65)])
def test_twin_per_step_launches(T, N, W, K, nonrev):
    """rollout_random(k) against rollout_random(k, per_step_launches=True) on a second env with the same seed."""
    tv, _ = T
    snaps = []
    for per_step in (False, True):
        env = tv.VecTron(N, W, seed=11, rank=4, obs_format="codes")
        env.reset()
        totals = torch.zeros(4, dtype=torch.int64, device="cuda")
        env.rollout_random(K, totals, nonreversing=nonrev, per_step_launches=per_step)
        torch.cuda.synchronize()
        st = env.state()
        snap = {"obs": np_(env.obs).copy(), "grid": np_(env.grid()).copy(), "totals": np_(totals).copy()}
        for k in STATE_KEYS:
            snap[k] = np_(st[k]).copy()
        snaps.append(snap)
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k], snaps[1][k]), k
