"""What the rollout tests (tests/test_gpu_rollout_*.py) share: the CPU oracle driven as a rollout drives the env, and the
comparisons of everything a caller can read back from a VecTron with that oracle and with a twin VecTron.  All comparisons
are exact.  A plain module, imported by name; torch is imported only by the functions that touch the GPU, so the
oracle-only parts work on a machine without one."""
import os

import numpy as np
import pytest

LAUNCH = 64                                                      # steps per persistent launch (TRON_ROLLOUT_CHUNK)
WALL, P1_HEAD = -1, 2                                            # raw tile values (map.py:9-17)
ORACLE_KEYS = ("obs", "grid", "pos", "alive", "dir", "done", "winner", "weight", "degree", "tick", "episode", "eplen")


def np_(t):
    return t.detach().cpu().numpy()


def tally(done, winner, stepped):
    """{env_steps, p1_wins, p2_wins, draws} of one step; `stepped`: the envs that were live when the step began (a
    finished env only restarts under autoreset: neither a step nor an ending)."""
    fin = (done == 1) & stepped
    return np.array([int(stepped.sum()), int((fin & (winner == 1)).sum()), int((fin & (winner == 2)).sum()),
                     int((fin & (winner == 0)).sum())], np.int64)


def oracle_obs(oracle, grid):
    """[N, 2, G]: both players' code planes of the oracle's boards."""
    return np.stack([oracle.state_for_player(grid, 1), oracle.state_for_player(grid, 2)], 1)


def gpu_modules(threads=None):
    """(tron.vec, oracle), or a skip without a GPU.  threads=True gives the oracle the host's cores, 16 at the most;
    restore_threads() takes them back."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tron.vec as tv
    import oracle
    if threads:
        oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
    return tv, oracle


def restore_threads(oracle):
    oracle.set_threads(1)


class Ref:
    """The CPU oracle stepped as the env is: totals that do not count a finished env's restart as a step, a log per
    launch of roll(), and, where asked for, a look at the finished boards before they restart.

    A step with autoreset is VecOracle.step(autoreset=True); with `events` or `before_restart` it is a step without
    autoreset and reset_masked(done) instead, which leaves the same state (tests/test_rollout_support_cpu.py)."""

    def __init__(self, oracle, N, W, seed, rank, fair=False, mode=None, reward=None, slide=None, events=False,
                 before_restart=None, at_launch=None):
        kw = dict(mode=mode, seed=seed, stream=rank, fair=fair)
        if reward is not None:
            kw["reward"] = reward
        if slide is not None:
            kw["slide"] = slide
        self.oracle, self.N, self.W, self.fair, self.seed, self.rank = oracle, N, W, fair, seed & 0xFFFFFFFF, rank
        self.v = oracle.VecOracle(N, W, **kw)
        self.v.reset_all()
        self.totals = np.zeros(4, np.int64)
        self.restarts_per_step = []                              # per step with autoreset: how many envs restarted
        self.launches = []                                       # per launch: ([N] episode before, [k, N] restarted in step s)
        self.launch_notes = []                                   # per launch: what at_launch(self) returned at its entry
        self.entered_done = 0                                    # envs that were finished when a launch began
        self.events, self.before_restart, self.at_launch = events, before_restart, at_launch
        S = W + 2
        b = np.zeros((S, S), bool)
        b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = True
        self.border = b.reshape(-1)
        self.border_deaths = 0                                   # episodes that ended with a head on a border cell
        self.same_cell = 0                                       # episodes that ended with both heads on one cell (P2's over P1's)
        self.long_episodes = 0                                   # episodes of 20 steps and more

    def step(self, actions=None, uniforms=None, nonrev=False, autoreset=True, count=True):
        """One step; returns done / winner / reward as the step reports them (with autoreset: before the restart)."""
        v = self.v
        stepped = v.done == 0
        by_hand = autoreset and (self.events or self.before_restart is not None)
        _, d, w, r = v.step(actions, uniforms, autoreset=autoreset and not by_hand, want_obs=False, nonreversing=nonrev)
        if count:
            self.totals += tally(d, w, stepped)
        fin = d == 1
        if autoreset:
            self.restarts_per_step.append(int(fin.sum()))
        if by_hand and fin.any():
            if self.events:
                g = v.grid[fin & stepped]
                self.border_deaths += int((g[:, self.border] != WALL).any(1).sum())
                self.same_cell += int((~(g == P1_HEAD).any(1)).sum())
                self.long_episodes += int((v.eplen[fin] >= 20).sum())
            if self.before_restart is not None:
                self.before_restart(self, fin)
            v.reset_masked(fin)
        return d, w, r

    def roll(self, K, nonrev=False):
        """K steps with autoreset, logged as the launches of at most LAUNCH steps that a rollout makes of them."""
        left = K
        while left:
            k = min(left, LAUNCH)
            before = self.v.episode.copy()
            if self.at_launch is not None:
                self.launch_notes.append(self.at_launch(self))
            self.entered_done += int((self.v.done == 1).sum())
            hit = np.zeros((k, self.N), bool)
            for s in range(k):
                ep = self.v.episode.copy()
                self.step(nonrev=nonrev)
                hit[s] = self.v.episode != ep
            self.launches.append((before, hit))
            left -= k

    def apply(self, op, nonrev=False):
        """("roll", K); ("steps", n): per-step launches with autoreset; ("steps_noreset", n): without.  Only a roll counts."""
        if op[0] == "roll":
            self.roll(op[1], nonrev)
        else:
            for _ in range(op[1]):
                self.step(nonrev=nonrev, autoreset=op[0] == "steps", count=False)

    def obs(self):
        return oracle_obs(self.oracle, self.v.grid)

    def snapshot(self, copy=True):
        """What check_against_oracle compares, as a dict; the copy stays as it is when the oracle steps on."""
        v = self.v
        out = dict(obs=self.obs(), totals=self.totals, **{k: getattr(v, k) for k in ORACLE_KEYS[1:]})
        return {k: a.copy() for k, a in out.items()} if copy else out

    def clashes(self, envs=16):
        """Among the first `envs` envs: (restarts inside the launches whose make_game clashes, those of them that are a
        launch's last or last but one game)."""
        nd = 9 if self.fair else 7                               # draws of a game without a clash
        inside = at_end = 0
        for before, hit in self.launches:
            for e in range(min(envs, self.N)):
                after = int(before[e]) + int(hit[:, e].sum())
                for ep in range(int(before[e]) + 1, after + 1):
                    # 48 words: the point, four starts, sixteen redraws of player 1, two weights and the degree are 41
                    words = np.concatenate([self.oracle.philox([e, ep, 2, b], [self.seed, self.rank]) for b in range(12)])
                    if self.oracle.make_game(self.W, self.fair, words)[3] > nd:
                        inside += 1
                        at_end += ep >= after - 1
        return inside, at_end


def make_tape(N, K, salt=0, lo=0, hi=4):
    """[K, N, 2] int8 actions on the device, uniform over lo..hi-1 from a seeded torch.Generator."""
    import torch
    g = torch.Generator().manual_seed(1_000_003 * N + 131 * K + salt)
    return torch.randint(lo, hi, (K, N, 2), generator=g, dtype=torch.int64).to(torch.int8).cuda()


def start_positions(rs, N, W):
    """[N, 4] int8 start positions from a RandomState, the two players of an env never on one cell."""
    sp = rs.randint(0, W, (N, 4)).astype(np.int8)
    clash = (sp[:, 0] == sp[:, 2]) & (sp[:, 1] == sp[:, 3])
    sp[clash, 3] = (sp[clash, 1] + 1) % W
    return sp


def new_totals():
    import torch
    return torch.zeros(4, dtype=torch.int64, device="cuda")


def step_counted(env, totals, actions, live=None):
    """One per-step launch with autoreset, the totals a rollout keeps of it (it counts the envs that move: every env,
    unless the caller says which were live when the step began), and clones of the (reward, done, winner) it returned."""
    import torch
    _, r, d, w = env.step(actions, autoreset=True)
    if live is None:
        live = torch.ones_like(d, dtype=torch.bool)
    fin = (d == 1) & live
    totals += torch.stack([live.sum(), (fin & (w == 1)).sum(), (fin & (w == 2)).sum(), (fin & (w == 0)).sum()])
    return r.clone(), d.clone(), w.clone()


def apply(env, totals, op, nonrev=False, per_step=False):
    """Ref.apply's ops on a VecTron."""
    if op[0] == "roll":
        env.rollout_random(op[1], totals, nonreversing=nonrev, per_step_launches=per_step)
    else:
        for _ in range(op[1]):
            env.step(autoreset=op[0] == "steps", nonreversing=nonrev)


def pull(env, totals=None):
    """Everything a caller can read back, on the host: obs [N, 2, G], grid [N, G], every field of state(), the totals."""
    import torch
    torch.cuda.synchronize()
    got = dict(obs=np_(env.obs).reshape(env.N, 2, -1).copy(), grid=np_(env.grid()).reshape(env.N, -1))
    if totals is not None:
        got["totals"] = np_(totals).copy()
    got.update({k: np_(v) for k, v in env.state().items()})
    return got


def check_against_oracle(got, ref, tag, totals=True):
    """pull()'s dict against a Ref, or against a Ref.snapshot() taken earlier; field by field."""
    exp = ref.snapshot(copy=False) if isinstance(ref, Ref) else ref
    c = got["counters"].astype(np.uint32)
    have = dict(got, tick=c[:, 0], episode=c[:, 1], eplen=c[:, 2])
    for k in ORACLE_KEYS + (("totals",) if totals else ()):
        assert have[k].shape == exp[k].shape and np.array_equal(have[k], exp[k]), (tag, k)


def check_against_twin(got, twin, tag, keys=None):
    """Two pull() dicts against each other, field by field: every field of both, or `keys`."""
    if keys is None:
        assert set(got) == set(twin), (tag, sorted(set(got) ^ set(twin)))
        keys = sorted(got)
    for k in keys:
        assert got[k].shape == twin[k].shape and np.array_equal(got[k], twin[k]), (tag, k)
