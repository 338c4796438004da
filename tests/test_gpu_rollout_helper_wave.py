"""k_obs_roll runs with a helper wave beside every game wave.  The helper draws the Philox words of the launch — every
step's action bits, and the start positions of every restart — into rings in LDS, in blocks of R = 8 steps with one
workgroup barrier per block; the game wave reads a byte per step and a dword per restart and draws nothing itself.  What
tron_rollout_random leaves behind must still be, bit for bit, what the CPU oracle stepped the same number of times holds
and what a twin VecTron run with one launch per step (per_step_launches=True: k_obs) holds: both observation planes, the
board, every field VecTron.state() shows (pos, alive, dir, done, winner, weight, degree, counters) and the totals, after
every call.  rs4's next-game words (nstart, nenvp) show as pos / weight / degree after the env's next restart, so every
sequence ends with per-step launches until every env has restarted again, compared with the oracle after each of them.

A sequence is one call per step count, one after the other, so that every launch but the first starts from what an
epilogue wrote and primes its rings from a new tick and episode: 1, R - 1, R, R + 1, 2R, 2R + 1 (the ring wraps, the last
block is partial), 63, 64, 65 (a launch of 64 and one of 1), 130 (64 + 64 + 2).
Envs: 1, 63, 64, 65, 130, 257 (one game wave and one helper per workgroup, ragged last waves); 16 384 + 1 and 16 384 + 200
(four game waves and four helpers per workgroup: 512 threads; a last workgroup of one env, and of three full waves and a
short one).  Sides 4 (a restart nearly every step, clashing starts), 10, 24 (the workload), 30 (three game waves, six in
all); `fair` on sides 4 and 10; both action policies.  A last sequence enters its launches with finished envs (steps
without autoreset in front): such an env restarts in a launch's first step without moving and draws its actions one tick
behind the others from then on.

test_inputs_reach_the_cases asserts, from the oracle alone, that these inputs reach the cases they are there for.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R = 8                                                            # steps per block of the helper (ROLL_R)
LAUNCH = 64                                                      # steps per persistent launch (TRON_ROLLOUT_CHUNK)
STEPS = (1, R - 1, R, R + 1, 2 * R, 2 * R + 1, 63, 64, 65, 130)
SMALL = (1, 63, 64, 65, 130, 257)
LARGE = (16384 + 1, 16384 + 200)
CASES = [(4, False), (10, False), (24, False), (30, False), (4, True), (10, True)]
LARGE_CASES = [(24, False), (30, False), (4, True)]
SEED, RANK = 0xB10C, 1
FOLLOW_MAX = 64                                                  # per-step launches after a sequence, at the most
STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree", "counters")
ROLLS = [("roll", k) for k in STEPS]
FINISHED = [("steps_noreset", 5), ("roll", 2 * R + 1), ("steps_noreset", 3), ("roll", 65), ("steps_noreset", 2), ("roll", 1),
            ("roll", R)]


@pytest.fixture(scope="module")
def T():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tron.vec as tv
    import oracle
    oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
    yield tv, oracle
    oracle.set_threads(1)


def np_(t):
    return t.detach().cpu().numpy()


class Ref:
    """The oracle stepped through a sequence, with what the conditions on the inputs need: per launch the episode
    counters around it, and per launch and step which envs restarted."""

    def __init__(self, oracle, N, W, fair):
        self.oracle, self.N, self.W, self.fair = oracle, N, W, fair
        self.v = oracle.VecOracle(N, W, seed=SEED, stream=RANK, fair=fair)
        self.v.reset_all()
        self.totals = np.zeros(4, np.int64)
        self.launches = []                                       # per launch: ([N] episode before, [k, N] restarted in step s)
        self.entered_done = 0                                    # envs that were finished when a launch began

    def step(self, nonrev, autoreset=True, count=True):
        v = self.v
        was_done = v.done == 1
        _, d, w, _ = v.step(autoreset=autoreset, want_obs=False, nonreversing=nonrev)
        if count:                                                # (a finished env restarts without stepping: not counted)
            stepped = ~was_done
            self.totals += [int(stepped.sum()), int((stepped & (d == 1) & (w == 1)).sum()),
                            int((stepped & (d == 1) & (w == 2)).sum()), int((stepped & (d == 1) & (w == 0)).sum())]

    def roll(self, K, nonrev):
        left = K
        while left:
            k = min(left, LAUNCH)
            before = self.v.episode.copy()
            self.entered_done += int((self.v.done == 1).sum())
            hit = np.zeros((k, self.N), bool)
            for s in range(k):
                ep = self.v.episode.copy()
                self.step(nonrev)
                hit[s] = self.v.episode != ep
            self.launches.append((before, hit))
            left -= k

    def apply(self, op, nonrev):
        if op[0] == "roll":
            self.roll(op[1], nonrev)
        else:
            for _ in range(op[1]):
                self.step(nonrev, autoreset=False, count=False)

    def obs(self):
        g = self.v.grid
        return np.stack([self.oracle.state_for_player(g, 1), self.oracle.state_for_player(g, 2)], 1)

    def clashes(self, envs=16):
        """Restarts inside the launches, among the first `envs` envs, whose make_game clashes."""
        nd = 9 if self.fair else 7                               # draws of a game without a clash
        n = 0
        for before, hit in self.launches:
            for e in range(min(envs, self.N)):
                for ep in range(int(before[e]) + 1, int(before[e]) + int(hit[:, e].sum()) + 1):
                    words = np.concatenate([self.oracle.philox([e, ep, 2, b], [SEED, RANK]) for b in range(12)])
                    n += self.oracle.make_game(self.W, self.fair, words)[3] > nd
        return n


def apply(env, totals, op, nonrev, per_step):
    if op[0] == "roll":
        env.rollout_random(op[1], totals, nonreversing=nonrev, per_step_launches=per_step)
    else:
        for _ in range(op[1]):
            env.step(autoreset=False, nonreversing=nonrev)


def pull(env, totals):
    torch.cuda.synchronize()
    got = dict(obs=np_(env.obs).reshape(env.N, 2, -1).copy(), grid=np_(env.grid()).reshape(env.N, -1),
               totals=np_(totals).copy())
    got.update({k: np_(v) for k, v in env.state().items()})
    return got


def check_against_oracle(got, ref, tag, totals=True):
    v = ref.v
    assert np.array_equal(got["obs"], ref.obs()), (tag, "obs")
    assert np.array_equal(got["grid"], v.grid), (tag, "grid")
    for k in ("pos", "alive", "dir", "done", "winner", "weight", "degree"):
        assert np.array_equal(got[k], getattr(v, k)), (tag, k)
    if totals:
        assert np.array_equal(got["totals"], ref.totals), (tag, "totals")
    c = got["counters"].astype(np.uint32)
    assert np.array_equal(c[:, 0], v.tick), (tag, "tick")
    assert np.array_equal(c[:, 1], v.episode), (tag, "episode")
    assert np.array_equal(c[:, 2], v.eplen), (tag, "eplen")


def check_against_twin(got, twin, tag):
    for k in ("obs", "grid", "totals") + STATE_KEYS:
        assert np.array_equal(got[k], twin[k]), (tag, k)


def make(tv, N, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    return env, torch.zeros(4, dtype=torch.int64, device="cuda")


def run_sequence(T, N, W, fair, nonrev, ops):
    tv, oracle = T
    ref = Ref(oracle, N, W, fair)
    env, totals = make(tv, N, W, fair)
    twin, ttot = make(tv, N, W, fair)
    for i, op in enumerate(ops):
        tag = (N, W, fair, nonrev, i, op)
        ref.apply(op, nonrev)
        apply(env, totals, op, nonrev, False)
        apply(twin, ttot, op, nonrev, True)
        got = pull(env, totals)
        check_against_oracle(got, ref, tag)
        check_against_twin(got, pull(twin, ttot), tag + ("twin",))
    # rs4.nstart / rs4.nenvp of every env: per-step launches with uniform actions until every env has restarted again
    seen = ref.v.episode.copy()
    for j in range(FOLLOW_MAX):
        if (ref.v.episode != seen).all():
            break
        ref.step(False, count=False)
        env.step()
        twin.step()
        check_against_oracle(pull(env, totals), ref, (N, W, fair, nonrev, "follow", j))
    assert (ref.v.episode != seen).all()                         # (the oracle alone) the next game of every env was looked at
    check_against_twin(pull(env, totals), pull(twin, ttot), (N, W, fair, nonrev, "follow", "twin"))
    env.close()
    twin.close()
    return ref


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N", SMALL)
@pytest.mark.parametrize("W,fair", CASES)
def test_one_game_wave_per_workgroup(T, W, fair, N, nonrev):
    ref = run_sequence(T, N, W, fair, nonrev, ROLLS)
    assert sum(int(hit.sum()) for _, hit in ref.launches) > N     # games ended and restarted inside the launches


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N", LARGE)
@pytest.mark.parametrize("W,fair", LARGE_CASES)
def test_four_game_waves_per_workgroup(T, W, fair, N, nonrev):
    """More 64-env waves than the chip has CUs: 256 envs per workgroup (192 at side 30), 512 threads (384)."""
    run_sequence(T, N, W, fair, nonrev, ROLLS)


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W,fair", [(4, False), (24, False), (10, True)])
def test_launches_entered_with_finished_envs(T, W, fair, nonrev):
    ref = run_sequence(T, 130, W, fair, nonrev, FINISHED)
    assert ref.entered_done > 0


def longest_run(hit):
    """The longest run of consecutive steps of one launch in which one env restarts."""
    best = 0
    run = np.zeros(hit.shape[1], np.int64)
    for s in range(hit.shape[0]):
        run = np.where(hit[s], run + 1, 0)
        best = max(best, int(run.max()))
    return best


def oracle_only(oracle, N, W, fair, nonrev, ops):
    ref = Ref(oracle, N, W, fair)
    for op in ops:
        ref.apply(op, nonrev)
    return ref


def test_inputs_reach_the_cases(T):
    """Conditions on the oracle alone (no GPU result enters): the sequences above reach what they are there to reach.
    Found for these seeds: the longest run of consecutive steps in which one env restarts is 15 at side 4 and 4 at side 24
    (uniform actions); one env restarts up to 8 times in one block of 8 steps at side 4 and 5 times at side 24."""
    _, oracle = T
    for W, least in ((4, 3), (24, 3)):
        ref = oracle_only(oracle, 130, W, False, False, ROLLS)
        assert max(longest_run(hit) for _, hit in ref.launches) >= least    # restarts in consecutive steps: the start ring's ordinals run ahead of the blocks
        first = sum(int(hit[0::R].sum()) for _, hit in ref.launches)
        last = sum(int(hit[R - 1::R].sum()) for _, hit in ref.launches)
        assert first > 0 and last > 0                            # a restart in the first and in the last step of a block
        most = max(int(hit[b:b + R, e].sum()) for _, hit in ref.launches if len(hit) >= R
                   for b in range(0, len(hit) - R + 1, R) for e in range(0, 130, 13))
        assert most >= 3                                         # one env, one block, three ordinals and more
    # an env that does not restart in a whole launch: of one block with uniform actions, of three with the non-reversing ones
    ref = oracle_only(oracle, 130, 24, False, False, ROLLS)
    assert any((hit.sum(0) == 0).any() for _, hit in ref.launches if len(hit) >= R)
    ref = oracle_only(oracle, 130, 24, False, True, ROLLS)
    assert any((hit.sum(0) == 0).any() for _, hit in ref.launches if len(hit) > 2 * R)
    for fair in (False, True):                                   # clashing starts at side 4: the helper's general routine
        assert oracle_only(oracle, 130, 4, fair, False, ROLLS).clashes() > 0
    ref = oracle_only(oracle, 130, 24, False, False, FINISHED)
    assert ref.entered_done > 0                                  # envs that are finished when a launch begins
