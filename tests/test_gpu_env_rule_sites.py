"""The five places a move is made share one copy of the rule (tron_device.hpp, "the rule"); what is left to each is its
glue — how it reads its cells, writes them, packs its records and rebuilds a restarted board.  A bug in a helper shows in
every kernel at once; this file is for a bug in ONE caller's glue: every path steps the same envs with the same actions
(and slide uniforms), and is compared with the CPU oracle and with the other paths of its mode after every step.

130 envs (two full waves and a ragged third of two lanes) on a 4x4 board, where collisions, head-ons and out-of-bounds
moves all come within a few steps; 12 steps, autoreset on, the reward table whose non-terminal reward is the step index
(so the eplen path is live).  No tolerances: every value is an integer or one of the table's floats.  The oracle's own
output is checked for the events the cases are there for, so a seed that stops producing them fails instead of passing
on nothing."""
import numpy as np
import pytest

from rollout_support import Ref, check_against_oracle, gpu_modules, new_totals, np_, pull

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# This seed, counted on the CPU with the oracle alone (oracle_run below), over the 12 steps of the 130 envs — mode None: 31
# same-cell head-ons, 14 swap-throughs, 797 moves off the board, 996 restarts; ice: 310 slides that land on the wall, 1 156
# restarts; temper: 111 and 1 040.
N, W, STEPS, SEED, RANK = 130, 4, 12, 20251, 7
SLIDE = 0.5
REWARD = dict(step=0.0, win=100.0, lose=-25.0, draw=0.0, step_is_index=1)      # DQN.py:224-241
STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree")


def inputs():
    rng = np.random.default_rng(SEED)
    return rng.integers(0, 4, (STEPS, N, 2)).astype(np.int8), rng.random((STEPS, N, 2), dtype=np.float32)


def oracle_run(oracle, mode):
    """The oracle through the 12 steps, autoreset done by hand so that the finished boards can be looked at: per step
    what a caller reads back, and the number of each event the cases are there for."""
    acts, unis = inputs()
    v = oracle.VecOracle(N, W, mode=mode, seed=SEED, stream=RANK, reward=REWARD, slide=SLIDE)
    v.reset_all()
    ev = dict(head_on=0, swap=0, off_board=0, slide_on_wall=0, restart=0)
    steps = []
    for s in range(STEPS):
        old = v.pos.astype(np.int32).copy()
        _, d, w, r = v.step(acts[s], None if mode is None else unis[s], autoreset=False, want_obs=False)
        new = v.pos.astype(np.int32)
        p1, p2, o1, o2 = new[:, 0:2], new[:, 2:4], old[:, 0:2], old[:, 2:4]
        off = np.stack([((p < 0) | (p >= W)).any(1) for p in (p1, p2)], 1)
        slid = np.stack([np.abs(p - o).sum(1) == 2 for p, o in ((p1, o1), (p2, o2))], 1)
        ev["head_on"] += int(((p1 == p2).all(1) & ~off[:, 0]).sum())
        ev["swap"] += int(((p1 == o2).all(1) & (p2 == o1).all(1)).sum())
        ev["off_board"] += int(off.sum())
        ev["slide_on_wall"] += int((slid & off).sum())
        ev["restart"] += int((d == 1).sum())
        v.reset_masked(d == 1)
        steps.append(dict(step_done=d.copy(), step_winner=w.copy(), reward=r.copy(), grid=v.grid.copy(),
                          counters=np.stack([v.tick, v.episode, v.eplen], 1).copy(),
                          **{k: getattr(v, k).copy() for k in STATE_KEYS}))
    return steps, ev


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules()
    return tv, oracle, {mode: oracle_run(oracle, mode) for mode in (None, "ice", "temper")}


def read_back(env, r, d, w):
    torch.cuda.synchronize()
    st = env.state()
    out = dict(step_done=np_(d).copy(), step_winner=np_(w).copy(), reward=np_(r).copy(), grid=np_(env.grid()).reshape(N, -1),
               counters=np_(st["counters"]).astype(np.uint32))
    out.update({k: np_(st[k]) for k in STATE_KEYS})
    return out


def same(a, b, tag):
    for k in b:
        assert np.array_equal(a[k], b[k]), f"{tag}: {k}"


PATHS = {                                        # the kernel a step goes through
    "obs": dict(obs_is_state=True),              # k_obs / k_obs_slide
    "board": dict(obs_is_state=False),           # k_tile
    "inc": dict(obs_is_state=True, incremental=True),   # k_inc
}


def test_the_seed_shows_every_event(T):
    ev = {mode: T[2][mode][1] for mode in T[2]}
    for k in ("head_on", "swap", "off_board", "restart"):
        assert ev[None][k] >= 1, (k, ev)
    for mode in ("ice", "temper"):
        assert ev[mode]["slide_on_wall"] >= 1 and ev[mode]["restart"] >= 1, (mode, ev)


@pytest.mark.parametrize("mode,paths", [(None, ("obs", "board", "inc")), ("ice", ("obs", "board")), ("temper", ("obs", "board"))])
def test_every_path_of_a_mode(T, mode, paths):
    tv, _, runs = T
    ref = runs[mode][0]
    acts, unis = inputs()
    envs = {}
    for p in paths:
        envs[p] = tv.VecTron(N, W, mode=mode, seed=SEED, rank=RANK, obs_format="codes", reward=REWARD, slide=SLIDE, **PATHS[p])
        assert envs[p].obs_is_state == PATHS[p]["obs_is_state"] and envs[p].incremental == (p == "inc")
        envs[p].reset()
    for s in range(STEPS):
        a = torch.from_numpy(acts[s])
        u = None if mode is None else torch.from_numpy(unis[s])
        got = {}
        for p in paths:
            _, r, d, w = envs[p].step(a, u, autoreset=True)
            got[p] = read_back(envs[p], r, d, w)
            same(got[p], ref[s], f"{mode} {p} against the oracle, step {s}")
        for p in paths[1:]:
            same(got[p], got[paths[0]], f"{mode} {p} against {paths[0]}, step {s}")


@pytest.mark.parametrize("mode,resident", [(None, False), ("temper", True)])      # k_obs_roll, k_obs_roll_slide
def test_rollout_in_one_launch(T, mode, resident):
    tv, oracle, _ = T
    env = tv.VecTron(N, W, mode=mode, seed=SEED, rank=RANK, obs_format="codes", reward=REWARD, slide=SLIDE)
    assert env.obs_is_state
    env.reset()
    ref = Ref(oracle, N, W, SEED, RANK, mode=mode, reward=REWARD, slide=SLIDE)
    for _ in range(STEPS):
        ref.step()
    assert ref.totals[1:].sum() >= 1              # somebody restarted inside the launch
    totals = new_totals()                         # {env_steps, p1_wins, p2_wins, draws}
    env.rollout_random(STEPS, totals, resident=resident)
    check_against_oracle(pull(env, totals), ref, (mode, resident))
