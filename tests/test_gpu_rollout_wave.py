"""The persistent rollout with one lane per env (k_obs_roll): a wave steps its own envs with no barrier, the boards sit
in LDS at 4 bits per cell, and the chunks a step stores come from a per-env 64-bit mask instead of a search.  What
that can get wrong: ragged waves and workgroups, the 64-step launch seam, the mask's width limit (cpe = 64 at W = 30;
wider boards must take the walking kernel), masks that grow over long episodes, masks rebuilt by the prologue after
every writer the API has changed the buffer, finished envs found at the start of a launch.

Every byte of env.obs, grid() and state() and the totals are compared with the CPU oracle driven the same way; no
tolerances.  tron_rollout_random implies autoreset and returns totals only, so done / winner / reward are compared
as the totals of every rollout and as the per-step arrays of the step() calls between rollouts; envs that finished
under autoreset=False reach the rollout as finished envs (nothing is redrawn for them before it)."""
import numpy as np
import pytest

from rollout_support import Ref, check_against_oracle, check_against_twin, gpu_modules, new_totals, np_, pull, restore_threads, \
    start_positions

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def T():
    return gpu_modules()


def check(env, ref, tag):
    """Every byte a caller can read back against the oracle."""
    check_against_oracle(pull(env), ref, tag, totals=False)


def rollout(env, ref, K, nonrev=False, tag=""):
    """K steps both ways; the rollout's totals against the oracle's."""
    totals = new_totals()
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
    return env, Ref(oracle, N, W, seed, rank, events=True)


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
    _, oracle = gpu_modules(threads=True)
    try:
        env, ref = make(T, N, 6, seed=N % 1000, rank=2)
        rollout(env, ref, 65)
        rollout(env, ref, 3)
    finally:
        restore_threads(oracle)


@pytest.mark.parametrize("W,K", [(30, 65), (32, 65), (9, 20)])
def test_mask_width_limits_and_routing(T, W, K):
    """W = 30: 64 chunks per board, the last mask that fits (bit 63 is the last row's chunk).  W = 32: 73 chunks, the host
    must route to k_obs_roll_walk.  W = 9: an odd side stays on the board-owning layout (k_tile_roll)."""
    tv, oracle = T
    N = 130
    env = tv.VecTron(N, W, seed=5, rank=3, obs_format="codes")
    assert env.obs_is_state == (W % 2 == 0)
    env.reset()
    ref = Ref(oracle, N, W, 5, 3, events=True)
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
        totals = new_totals()
        env.rollout_random(K, totals, nonreversing=nonrev, per_step_launches=per_step)
        snaps.append(pull(env, totals))
    check_against_twin(snaps[0], snaps[1], "per_step_launches")
