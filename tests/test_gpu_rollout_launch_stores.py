"""k_obs_roll writes an env's observation planes once per persistent launch (the chunks its steps touched, from the boards in
LDS, in the epilogue) instead of once per step.  What tron_rollout_random leaves behind must be, bit for bit, what the CPU
oracle stepped the same number of times holds, and what a twin VecTron of the same seed run with one launch per step
(per_step_launches=True: k_obs, which stores every step) holds: both observation planes, the board, the state words as far as
VecTron.state() shows them (st4: pos, alive, dir, done, winner, tick, eplen; rs4: weight, degree, episode; the next start in
rs4 shows in every later restart), and the totals.

Shapes are the smallest at which this kernel takes another path: widths 4 (G = 36: two whole chunks and a short one of 4
cells, restarts nearly every step), 10 (G = 144: nine whole chunks), 24 (G = 676: short chunk of 4) and 30 (G = 1 024: 64
chunks, every bit of the masks, three waves per workgroup); 1, 63, 130 (a partly filled third wave) and 257 envs (a second
workgroup with one env); 1, 2, 63, 64, 65 (the launch split at 64) and 130 steps (three launches: the second and third
prologue rebuild the masks from what the epilogue before wrote); both action distributions.

The whole observation buffer [N, 2, G] is compared, so a store past G of a short last chunk — the first bytes of the
player-2 plane, or of the next env's player-1 plane — shows as a difference there: no separate check of the bytes between
planes is needed.
"""
import numpy as np
import pytest

from rollout_support import Ref, check_against_oracle, check_against_twin, gpu_modules, new_totals, np_, pull, restore_threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = (4, 10, 24, 30)
ENVS = (1, 63, 130, 257)
STEPS = (1, 2, 63, 64, 65, 130)
SEED, RANK = 0xC0FFEE, 2


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


_REFS = {}


def reference(oracle, N, W, nonrev):
    """The oracle's snapshots after each step count of STEPS: computed once per (N, W, distribution), never modified."""
    key = (N, W, nonrev)
    if key not in _REFS:
        ref = Ref(oracle, N, W, SEED, RANK)
        snaps = {}
        for k in range(1, max(STEPS) + 1):
            ref.step(nonrev=nonrev)
            if k in STEPS:
                snaps[k] = ref.snapshot()
        _REFS[key] = snaps
    return _REFS[key]


def swap_codes(plane):
    """swap_codes4 on the host: the player-2 view of a player-1 plane (bodies -2 <-> -3, heads 10 <-> -10)."""
    table = np.arange(256, dtype=np.uint8).view(np.int8).copy()
    for a, b in ((-2, -3), (10, -10)):
        table[a & 0xFF], table[b & 0xFF] = b, a
    return table[plane.view(np.uint8)]


def check(got, exp, tag):
    check_against_oracle(got, exp, tag)
    assert np.array_equal(got["obs"][:, 1], swap_codes(got["obs"][:, 0])), (tag, "player-2 plane")


def make(tv, N, W):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes")
    assert env.obs_is_state
    env.reset()
    return env, new_totals()


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N", ENVS)
@pytest.mark.parametrize("W", WIDTHS)
def test_launch_stores_equal_oracle_and_per_step_twin(T, W, N, nonrev):
    """(a) the oracle, (b) the per-step twin, and the resident=True flag, after every step count of STEPS from a fresh reset."""
    tv, oracle = T
    snaps = reference(oracle, N, W, nonrev)
    for K in STEPS:
        env, totals = make(tv, N, W)
        env.rollout_random(K, totals, nonreversing=nonrev)
        got = pull(env, totals)
        check(got, snaps[K], (W, N, nonrev, K))
        twin, ttot = make(tv, N, W)
        twin.rollout_random(K, ttot, nonreversing=nonrev, per_step_launches=True)
        check_against_twin(got, pull(twin, ttot), (W, N, nonrev, K, "twin"))
        res, rtot = make(tv, N, W)
        res.rollout_random(K, rtot, nonreversing=nonrev, resident=True)
        check_against_twin(got, pull(res, rtot), (W, N, nonrev, K, "resident"))
        for e in (env, twin, res):
            e.close()
    assert int(snaps[max(STEPS)]["episode"].max()) > 3          # games ended and restarted inside the launches


@pytest.mark.parametrize("masked_reset", [False, True])
@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W", WIDTHS)
def test_launch_stores_between_other_writers(T, W, nonrev, masked_reset):
    """rollout_random(5), a step with explicit actions (k_obs), optionally a masked reset (k_obs_reset), rollout_random(70):
    the prologue reads what the other writers left, and they read what the epilogue left.  Compared with the oracle and the
    per-step twin after every call."""
    tv, oracle = T
    N = 130
    rng = np.random.RandomState(1000 + W)
    ref = Ref(oracle, N, W, SEED, RANK)
    env, totals = make(tv, N, W)
    twin, ttot = make(tv, N, W)

    def rollout(K, tag):
        env.rollout_random(K, totals, nonreversing=nonrev)
        twin.rollout_random(K, ttot, nonreversing=nonrev, per_step_launches=True)
        for k in range(K):
            ref.step(nonrev=nonrev)
        got = pull(env, totals)
        check(got, ref, (W, nonrev, masked_reset, tag))
        check_against_twin(got, pull(twin, ttot), (W, nonrev, masked_reset, tag, "twin"))

    rollout(5, "first rollout")
    a = rng.randint(0, 4, size=(N, 2)).astype(np.int8)
    dd, ww, _ = ref.step(a, count=False)
    o = ref.obs()
    for name, e in (("env", env), ("twin", twin)):
        obs, _, d, w = e.step(torch.from_numpy(a), autoreset=True)
        assert np.array_equal(np_(obs).reshape(N, 2, -1), o), (W, nonrev, masked_reset, name, "step obs")
        assert np.array_equal(np_(d), dd) and np.array_equal(np_(w), ww), (W, nonrev, masked_reset, name, "step done / winner")
    if masked_reset:
        mask = (rng.rand(N) < 0.5).astype(np.int8)
        mask[0] = 1
        for e in (env, twin):
            e.reset(mask=torch.from_numpy(mask))
        ref.v.reset_masked(mask)
    rollout(70, "second rollout")
    env.close()
    twin.close()
