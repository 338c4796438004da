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

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "deep-q-learning_tron_amd")


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tron.vec as tv
    import oracle
    return tv, oracle


def np_(t):
    return t.detach().cpu().numpy()


STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree", "counters")


def _snapshot(env):
    """Every byte a caller can read back: planes, board image, state words."""
    st = env.state()
    snap = {"obs": np_(env.obs).copy(), "grid": np_(env.grid()).copy()}
    for k in STATE_KEYS:
        snap[k] = np_(st[k]).copy()
    return snap


def _same(a, b, tag):
    for k in a:
        assert np.array_equal(a[k], b[k]), (tag, k)


def _against_oracle(snap, ref, o, tag):
    N = ref.N
    if o is not None:
        assert np.array_equal(snap["obs"].reshape(N, 2, -1), o), tag
    assert np.array_equal(snap["grid"].reshape(N, -1), ref.grid), tag
    assert np.array_equal(snap["pos"], ref.pos) and np.array_equal(snap["alive"], ref.alive), tag
    assert np.array_equal(snap["dir"], ref.dir), tag
    assert np.array_equal(snap["done"], ref.done) and np.array_equal(snap["winner"], ref.winner), tag
    assert np.array_equal(snap["weight"], ref.weight) and np.array_equal(snap["degree"], ref.degree), tag
    c = snap["counters"].astype(np.uint32)
    assert np.array_equal(c[:, 0], ref.tick) and np.array_equal(c[:, 1], ref.episode), tag
    assert np.array_equal(c[:, 2], ref.eplen), tag


def _tally(d, w, N):
    return np.array([N, int(((d == 1) & (w == 1)).sum()), int(((d == 1) & (w == 2)).sum()), int(((d == 1) & (w == 0)).sum())],
                    np.int64)


def _run_case(tv, oracle, N, W, K, nonrev, after=12, seed=77, rank=3):
    env = tv.VecTron(N, W, seed=seed, rank=rank, obs_format="codes")
    one = tv.VecTron(N, W, seed=seed, rank=rank, obs_format="codes")
    assert env.obs_is_state and one.obs_is_state
    ref = oracle.VecOracle(N, W, seed=seed, stream=rank)
    env.reset()
    one.reset()
    ref.reset_all()
    totals = torch.zeros(4, dtype=torch.int64, device="cuda")
    env.rollout_random(K, totals, nonreversing=nonrev)
    exp_gpu = np.zeros(4, np.int64)
    exp_ref = np.zeros(4, np.int64)
    o = None
    for k in range(K):
        _, _, d, w = one.step(nonreversing=nonrev)                   # K launches of the per-step kernel
        exp_gpu += _tally(np_(d), np_(w), N)
        o, d, w, _ = ref.step(autoreset=True, nonreversing=nonrev, want_obs=(k == K - 1))
        exp_ref += _tally(d, w, N)
    torch.cuda.synchronize()
    snap = _snapshot(env)
    _same(snap, _snapshot(one), "rollout vs per-step launches")
    _against_oracle(snap, ref, o, "rollout vs oracle")
    assert np.array_equal(np_(totals), exp_gpu) and np.array_equal(exp_gpu, exp_ref)
    # the next starts (rs4) show when envs restart: step on through restarts, both ways
    for k in range(after):
        env.step(nonreversing=nonrev)
        o, _, _, _ = ref.step(autoreset=True, nonreversing=nonrev, want_obs=(k == after - 1))
    if after:
        _against_oracle(_snapshot(env), ref, o, "steps after the rollout")
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
    oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
    try:
        _run_case(tv, oracle, 65536, 24, 70, False, after=2, seed=5, rank=1)
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("N,W", [(33, 10), (1000, 24), (4096, 24)])
def test_hand_off_through_memory(T, N, W):
    """rollout, a step with the caller's actions, rollout again: each launch finds in memory what the one before left."""
    tv, oracle = T
    env = tv.VecTron(N, W, seed=19, rank=4, obs_format="codes")
    ref = oracle.VecOracle(N, W, seed=19, stream=4)
    env.reset()
    ref.reset_all()
    rs = np.random.RandomState(11)
    o = None
    for K in (65, 2, 20):
        env.rollout_random(K)
        for _ in range(K):
            o, _, _, _ = ref.step(autoreset=True)
        _against_oracle(_snapshot(env), ref, o, f"rollout of {K}")
        for _ in range(3):
            acts = rs.randint(0, 4, (N, 2)).astype(np.int8)
            obs, reward, done, winner = env.step(torch.from_numpy(acts).cuda())
            o, d, w, r = ref.step(acts, autoreset=True)
            assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
            _against_oracle(_snapshot(env), ref, o, f"step with actions after rollout of {K}")


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N,W,K", [(1, 10, 20), (31, 24, 65), (1000, 24, 130), (4096, 32, 64), (65536, 24, 20)])
def test_resident_flag_gives_the_same_bytes(T, N, W, K, nonrev):
    tv, _ = T
    snaps = []
    for resident in (False, True):
        env = tv.VecTron(N, W, seed=3, rank=2, obs_format="codes")
        env.reset()
        totals = torch.zeros(4, dtype=torch.int64, device="cuda")
        env.rollout_random(K, totals, nonreversing=nonrev, resident=resident)
        snap = _snapshot(env)
        snap["totals"] = np_(totals).copy()
        snaps.append(snap)
    _same(snaps[0], snaps[1], "resident=True vs default")


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
        ref = oracle.VecOracle(N, W, seed=23, stream=5)
        env.reset()
        ref.reset_all()
        totals = torch.zeros(4, dtype=torch.int64, device="cuda")
        env.rollout_random(K, totals, nonreversing=nonrev)
        exp = np.zeros(4, np.int64)
        o = None
        for _ in range(K):
            o, d, w, _ = ref.step(autoreset=True, nonreversing=nonrev)
            exp += _tally(d, w, N)
        snap = _snapshot(env)
        walk = {k: got[f"{i}_{k}"] for k in snap}
        _same(walk, snap, f"walking grid vs default, case {i}")
        _against_oracle(walk, ref, o, f"walking grid vs oracle, case {i}")
        assert np.array_equal(got[f"{i}_totals"], exp) and np.array_equal(np_(totals), exp)
