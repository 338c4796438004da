"""The persistent rollout of the observation-is-state kernel (k_obs_roll) reads memory in the first step of a
launch only: boards, st4, rs4 and the fresh-board template are carried in LDS from step to step.  Everything a
caller can see afterwards — both observation planes, the board image, the st4-derived read-backs (positions,
alive, headings, done / winner, tick / episode / episode length), the rs4-derived ones (weights, degree, the
next starts: checked by stepping on through restarts) and the totals — must equal K launches of the per-step
kernel and K steps of the CPU oracle, byte for byte.  No tolerances anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from rollout_support import Ref, check_against_oracle, check_against_twin, gpu_modules, new_totals, np_, pull, restore_threads, \
    tally

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-q-learning_tron_amd")


@pytest.fixture(scope="module")
def T():
    return gpu_modules()


STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree", "counters")


def _run_case(tv, oracle, N, W, K, nonrev, after=12, seed=77, rank=3):
    env = tv.VecTron(N, W, seed=seed, rank=rank, obs_format="codes")
    one = tv.VecTron(N, W, seed=seed, rank=rank, obs_format="codes")
    assert env.obs_is_state and one.obs_is_state
    ref = Ref(oracle, N, W, seed, rank)
    env.reset()
    one.reset()
    totals = new_totals()
    env.rollout_random(K, totals, nonreversing=nonrev)
    exp_gpu = np.zeros(4, np.int64)
    for k in range(K):
        _, _, d, w = one.step(nonreversing=nonrev)                   # K launches of the per-step kernel
        exp_gpu += tally(np_(d), np_(w), np.ones(N, bool))
        ref.step(nonrev=nonrev)
    snap = pull(env, totals)
    check_against_twin(snap, pull(one), "rollout vs per-step launches", keys=("obs", "grid") + STATE_KEYS)
    check_against_oracle(snap, ref, "rollout vs oracle")
    assert np.array_equal(snap["totals"], exp_gpu)
    # the next starts (rs4) show when envs restart: step on through restarts, both ways
    for k in range(after):
        env.step(nonreversing=nonrev)
        ref.step(nonrev=nonrev, count=False)
    if after:
        check_against_oracle(pull(env, totals), ref, "steps after the rollout")
    return env, ref


# launch and chunk seams (64 steps per launch): 1 (per-step path), 2, one short launch, 63 / 64 / 65, two launches and a bit
KS = [1, 2, 20, 63, 64, 65, 130]
# one env, a tile less / more than one env (32-env tiles), a ragged last tile, whole tiles
NS = [1, 31, 33, 1000, 4096]


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W", [10, 24, 32])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_rollout_equals_per_step_launches_and_oracle(T, K, N, W, nonrev):
    tv, oracle = T
    _run_case(tv, oracle, N, W, K, nonrev, after=12 if N <= 1000 else 4)


def test_rollout_at_65536(T):
    """The benchmarked batch: 2 048 workgroups, more than the chip holds at once; a launch of 64 steps and one of 6."""
    tv, oracle = T
    gpu_modules(threads=True)
    try:
        _run_case(tv, oracle, 65536, 24, 70, False, after=2, seed=5, rank=1)
    finally:
        restore_threads(oracle)


@pytest.mark.parametrize("N,W", [(33, 10), (1000, 24), (4096, 24)])
def test_hand_off_through_memory(T, N, W):
    """rollout, a step with the caller's actions, rollout again: each launch finds in memory what the one before left."""
    tv, oracle = T
    env = tv.VecTron(N, W, seed=19, rank=4, obs_format="codes")
    ref = Ref(oracle, N, W, 19, 4)
    env.reset()
    rs = np.random.RandomState(11)
    for K in (65, 2, 20):
        env.rollout_random(K)
        for _ in range(K):
            ref.step()
        check_against_oracle(pull(env), ref, f"rollout of {K}", totals=False)
        for _ in range(3):
            acts = rs.randint(0, 4, (N, 2)).astype(np.int8)
            obs, reward, done, winner = env.step(torch.from_numpy(acts).cuda())
            d, w, r = ref.step(acts)
            assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
            check_against_oracle(pull(env), ref, f"step with actions after rollout of {K}", totals=False)


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N,W,K", [(1, 10, 20), (31, 24, 65), (1000, 24, 130), (4096, 32, 64), (65536, 24, 20)])
def test_resident_flag_gives_the_same_bytes(T, N, W, K, nonrev):
    tv, _ = T
    snaps = []
    for resident in (False, True):
        env = tv.VecTron(N, W, seed=3, rank=2, obs_format="codes")
        env.reset()
        totals = new_totals()
        env.rollout_random(K, totals, nonreversing=nonrev, resident=resident)
        snaps.append(pull(env, totals))
    check_against_twin(snaps[0], snaps[1], "resident=True vs default")


CHILD = r"""
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
import numpy as np, torch
import tron.vec as tv
out = {{}}
for i, (N, W, K, nonrev) in enumerate({cases!r}):
    env = tv.VecTron(N, W, seed=23, rank=5, obs_format="codes")
    env.reset()
    totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    env.rollout_random(K, totals, nonreversing=nonrev)
    st = env.state()
    out[f"{{i}}_obs"] = env.obs.cpu().numpy()
    out[f"{{i}}_grid"] = env.grid().cpu().numpy()
    out[f"{{i}}_totals"] = totals.cpu().numpy()
    for k in {keys!r}:
        out[f"{{i}}_{{k}}"] = st[k].cpu().numpy()
np.savez({path!r}, **out)
"""


def test_walking_fallback_in_a_child_process(T, tmp_path):
    """TRON_ROLL_GRID (read once per process): fewer workgroups than tiles, each walking several tiles and reading its
    state from memory at every step (k_obs_roll_walk).  Same bytes as the default of this process and as the oracle."""
    tv, oracle = T
    cases = [(1000, 24, 65, False), (4096, 10, 20, True), (33, 32, 130, False)]
    path = str(tmp_path / "walk.npz")
    code = CHILD.format(root=ROOT, pkg=PKG, cases=cases, keys=STATE_KEYS, path=path)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code]
    subprocess.run(cmd, env=dict(os.environ, TRON_ROLL_GRID="3"), check=True, timeout=600)
    got = np.load(path)
    for i, (N, W, K, nonrev) in enumerate(cases):
        env = tv.VecTron(N, W, seed=23, rank=5, obs_format="codes")
        ref = Ref(oracle, N, W, 23, 5)
        env.reset()
        totals = new_totals()
        env.rollout_random(K, totals, nonreversing=nonrev)
        for _ in range(K):
            ref.step(nonrev=nonrev)
        snap = pull(env, totals)
        walk = {k: got[f"{i}_{k}"] for k in ("totals",) + STATE_KEYS}
        walk.update(obs=got[f"{i}_obs"].reshape(N, 2, -1), grid=got[f"{i}_grid"].reshape(N, -1))
        check_against_twin(walk, snap, f"walking grid vs default, case {i}", keys=sorted(walk))
        check_against_oracle(walk, ref, f"walking grid vs oracle, case {i}")
        check_against_oracle(snap, ref, f"default vs oracle, case {i}")
