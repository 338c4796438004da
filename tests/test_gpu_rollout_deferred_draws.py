"""k_obs_roll draws a restarted env's next START POSITIONS in its step loop and nothing else: the weights and the degree of
the games it starts (rs4.envp / rs4.nenvp) are read by no step of mode None, so they are drawn once, in the launch's
epilogue, from the env's final episode counter and from how often the env restarted in the launch (0, 1, 2 or more).
What tron_rollout_random leaves behind must still be, bit for bit, what the CPU oracle stepped the same number of times
holds and what a twin VecTron run with one launch per step (per_step_launches=True: k_obs) holds: both observation
planes, the board, every field VecTron.state() shows and the totals, after every call.

rs4's four words are {envp, episode, nstart, nenvp}.  envp (weight, degree) and episode are read back by state() at
once; nstart and nenvp are the NEXT game's and show as pos / weight / degree after the env's next restart, so every
sequence ends with per-step launches (k_obs, which rotates the words as it always did) until every env has restarted
again, compared with the oracle after each of them.

Shapes: sides 4 (restarts nearly every step, clashing starts), 6, 10, 24 (the workload), 30 (64 chunks per env); 130 envs
(two full waves and a short one); calls of 1, 2, 3, 64, 65 and 64 steps one after the other, so that every launch but the
first starts from what an epilogue wrote (65 is a launch of 64 and one of 1); `fair` 0 and 1; both action distributions.
A second sequence puts per-step steps, tron_reset with an env mask, tron_reset with start_pos and
tron_set_weight_degree between the rollouts.

test_inputs_reach_the_cases asserts, from the oracle alone, that these inputs reach the cases they are there for.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDES = (4, 6, 10, 24, 30)
N = 130
LAUNCH = 64                                                      # steps per persistent launch (TRON_ROLLOUT_CHUNK)
SEED, RANK = 0xD1CE, 3
FOLLOW_MAX = 48                                                  # per-step launches after a sequence, at the most
STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree", "counters")
ROLLS = [("roll", 1), ("roll", 2), ("roll", 3), ("roll", 64), ("roll", 65), ("roll", 64)]
MIXED = [("steps", 5), ("roll", 3), ("reset_mask",), ("roll", 64), ("reset_pos",), ("roll", 2), ("set_wd",), ("roll", 1),
         ("set_wd",), ("roll", 65), ("steps", 2), ("roll", 64)]


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


def op_inputs(W, fair, i):
    """The host-side inputs of op number i of a sequence: the same for the env, its twin and the oracle."""
    rs = np.random.RandomState(1000 * W + 10 * i + int(fair))
    m = (rs.rand(N) < 0.4).astype(np.int8)
    m[0], m[64], m[N - 1] = 1, 0, 1
    sp = rs.randint(0, W, (N, 4)).astype(np.int8)
    clash = (sp[:, 0] == sp[:, 2]) & (sp[:, 1] == sp[:, 3])
    sp[clash, 3] = (sp[clash, 1] + 1) % W
    wt = rs.randint(40, 102, (N, 2)).astype(np.int16)
    dg = rs.randint(-30, 31, N).astype(np.int16)
    return m, sp, wt, dg


class Ref:
    """The oracle stepped through a sequence, with what the conditions on the inputs need: per launch and env the number
    of restarts, and whether an env restarted in two consecutive steps of one launch."""

    def __init__(self, oracle, W, fair):
        self.oracle, self.W, self.fair = oracle, W, fair
        self.v = oracle.VecOracle(N, W, seed=SEED, stream=RANK, fair=fair)
        self.v.reset_all()
        self.totals = np.zeros(4, np.int64)
        self.restarts = []                                       # per launch: [N] restarts inside it
        self.episodes = []                                       # per launch: ([N] episode before, [N] episode after)
        self.lengths = []                                        # per launch: its steps
        self.consecutive = 0

    def step(self, nonrev, count=True):
        v = self.v
        _, d, w, _ = v.step(autoreset=True, want_obs=False, nonreversing=nonrev)
        if count:
            self.totals += [v.N, int(((d == 1) & (w == 1)).sum()), int(((d == 1) & (w == 2)).sum()),
                            int(((d == 1) & (w == 0)).sum())]
        return d == 1                                            # (autoreset: a finished env restarted in this step)

    def roll(self, K, nonrev):
        left = K
        while left:
            k = min(left, LAUNCH)
            before = self.v.episode.copy()
            last = np.zeros(N, bool)
            for _ in range(k):
                r = self.step(nonrev)
                self.consecutive += int((r & last).sum())
                last = r
            self.restarts.append((self.v.episode - before).astype(np.int64))
            self.episodes.append((before, self.v.episode.copy()))
            self.lengths.append(k)
            left -= k

    def apply(self, op, i, nonrev):
        m, sp, wt, dg = op_inputs(self.W, self.fair, i)
        if op[0] == "roll":
            self.roll(op[1], nonrev)
        elif op[0] == "steps":
            for _ in range(op[1]):
                self.step(nonrev, count=False)
        elif op[0] == "reset_mask":
            self.v.reset_masked(m)
        elif op[0] == "reset_pos":
            self.v.set_starts(sp, mask=m)
        else:
            self.v.weight[:] = wt
            self.v.degree[:] = dg

    def obs(self):
        g = self.v.grid
        return np.stack([self.oracle.state_for_player(g, 1), self.oracle.state_for_player(g, 2)], 1)

    def clashes(self, envs=16):
        """Among the first `envs` envs: (restarts inside the launches whose make_game clashes, those of them that are a
        launch's last or last but one game: the ones the epilogue draws again in full)."""
        nd = 9 if self.fair else 7                               # draws of a game without a clash
        inside = at_end = 0
        for before, after in self.episodes:
            for e in range(envs):
                for ep in range(int(before[e]) + 1, int(after[e]) + 1):
                    # 48 words: the point, four starts, sixteen redraws of player 1, two weights and the degree are 41
                    words = np.concatenate([self.oracle.philox([e, ep, 2, b], [SEED, RANK]) for b in range(12)])
                    if self.oracle.make_game(self.W, self.fair, words)[3] > nd:
                        inside += 1
                        at_end += ep >= int(after[e]) - 1
        return inside, at_end


def apply(env, totals, op, i, W, fair, nonrev, per_step):
    m, sp, wt, dg = op_inputs(W, fair, i)
    if op[0] == "roll":
        env.rollout_random(op[1], totals, nonreversing=nonrev, per_step_launches=per_step)
    elif op[0] == "steps":
        for _ in range(op[1]):
            env.step(nonreversing=nonrev)
    elif op[0] == "reset_mask":
        env.reset(mask=torch.from_numpy(m))
    elif op[0] == "reset_pos":
        env.reset(mask=torch.from_numpy(m), start_pos=torch.from_numpy(sp))
    else:
        env.set_weight_degree(torch.from_numpy(wt), torch.from_numpy(dg))


def pull(env, totals):
    torch.cuda.synchronize()
    got = dict(obs=np_(env.obs).reshape(env.N, 2, -1).copy(), grid=np_(env.grid()).reshape(env.N, -1),
               totals=np_(totals).copy())
    got.update({k: np_(v) for k, v in env.state().items()})
    return got


def check_against_oracle(got, ref, tag):
    v = ref.v
    assert np.array_equal(got["obs"], ref.obs()), (tag, "obs")
    assert np.array_equal(got["grid"], v.grid), (tag, "grid")
    for k in ("pos", "alive", "dir", "done", "winner", "weight", "degree"):
        assert np.array_equal(got[k], getattr(v, k)), (tag, k)
    assert np.array_equal(got["totals"], ref.totals), (tag, "totals")
    c = got["counters"].astype(np.uint32)
    assert np.array_equal(c[:, 0], v.tick), (tag, "tick")
    assert np.array_equal(c[:, 1], v.episode), (tag, "episode")
    assert np.array_equal(c[:, 2], v.eplen), (tag, "eplen")


def check_against_twin(got, twin, tag):
    for k in ("obs", "grid", "totals") + STATE_KEYS:
        assert np.array_equal(got[k], twin[k]), (tag, k)


def make(tv, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    return env, torch.zeros(4, dtype=torch.int64, device="cuda")


def run_sequence(T, W, fair, nonrev, ops):
    tv, oracle = T
    ref = Ref(oracle, W, fair)
    env, totals = make(tv, W, fair)
    twin, ttot = make(tv, W, fair)
    for i, op in enumerate(ops):
        tag = (W, fair, nonrev, i, op)
        ref.apply(op, i, nonrev)
        apply(env, totals, op, i, W, fair, nonrev, False)
        apply(twin, ttot, op, i, W, fair, nonrev, True)
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
        check_against_oracle(pull(env, totals), ref, (W, fair, nonrev, "follow", j))
    assert (ref.v.episode != seen).all()                         # (the oracle alone) the next game of every env was looked at
    check_against_twin(pull(env, totals), pull(twin, ttot), (W, fair, nonrev, "follow", "twin"))
    env.close()
    twin.close()
    return ref


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("W", SIDES)
def test_consecutive_rollouts_equal_oracle_and_per_step_twin(T, W, fair, nonrev):
    ref = run_sequence(T, W, fair, nonrev, ROLLS)
    assert sum(int(r.sum()) for r in ref.restarts) > N           # games ended and restarted inside the launches


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W,fair", [(4, False), (4, True), (10, True), (24, False), (30, False)])
def test_rollouts_between_the_other_writers(T, W, fair, nonrev):
    """Rollouts after per-step k_obs steps, after tron_reset with an env mask, after tron_reset with start_pos and after
    tron_set_weight_degree (what it puts into rs4.envp stays until the env's first restart, then the launch's own draw)."""
    run_sequence(T, W, fair, nonrev, MIXED)


def oracle_only(oracle, W, fair, nonrev, ops):
    ref = Ref(oracle, W, fair)
    for i, op in enumerate(ops):
        ref.apply(op, i, nonrev)
    return ref


@pytest.mark.parametrize("ops", [ROLLS, MIXED], ids=["rolls", "mixed"])
def test_inputs_reach_the_cases(T, ops):
    """Conditions on the oracle alone (no GPU result enters): the sequences above reach what they are there to reach."""
    _, oracle = T
    for W in (4, 24):
        ref = oracle_only(oracle, W, False, False, ops)
        r = np.concatenate(ref.restarts)
        assert (r == 0).sum() > 0 and (r == 1).sum() > 0 and (r == 2).sum() > 0 and (r >= 3).sum() > 0
        assert ref.consecutive > 0                               # an env restarts in two consecutive steps of one launch
    for fair in (False, True):                                   # clashing starts: side 4, and `fair`
        inside, at_end = oracle_only(oracle, 4, fair, False, ops).clashes()
        assert inside > 0 and at_end > 0
    # a launch of one step holds envs with no restart and envs with one; set_weight_degree's values must survive in the former
    ref = oracle_only(oracle, 24, False, False, ops)
    one = [x for x, k in zip(ref.restarts, ref.lengths) if k == 1]
    assert one and all((x == 0).any() and (x == 1).any() for x in one)
