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
import numpy as np
import pytest

from rollout_support import Ref, apply, check_against_oracle, check_against_twin, gpu_modules, new_totals, pull, \
    restore_threads, start_positions

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIDES = (4, 6, 10, 24, 30)
N = 130
SEED, RANK = 0xD1CE, 3
FOLLOW_MAX = 48                                                  # per-step launches after a sequence, at the most
ROLLS = [("roll", 1), ("roll", 2), ("roll", 3), ("roll", 64), ("roll", 65), ("roll", 64)]
MIXED = [("steps", 5), ("roll", 3), ("reset_mask",), ("roll", 64), ("reset_pos",), ("roll", 2), ("set_wd",), ("roll", 1),
         ("set_wd",), ("roll", 65), ("steps", 2), ("roll", 64)]


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


def op_inputs(W, fair, i):
    """The host-side inputs of op number i of a sequence: the same for the env, its twin and the oracle."""
    rs = np.random.RandomState(1000 * W + 10 * i + int(fair))
    m = (rs.rand(N) < 0.4).astype(np.int8)
    m[0], m[64], m[N - 1] = 1, 0, 1
    sp = start_positions(rs, N, W)
    wt = rs.randint(40, 102, (N, 2)).astype(np.int16)
    dg = rs.randint(-30, 31, N).astype(np.int16)
    return m, sp, wt, dg


def ref_apply(ref, op, i, nonrev):
    m, sp, wt, dg = op_inputs(ref.W, ref.fair, i)
    if op[0] in ("roll", "steps"):
        ref.apply(op, nonrev)
    elif op[0] == "reset_mask":
        ref.v.reset_masked(m)
    elif op[0] == "reset_pos":
        ref.v.set_starts(sp, mask=m)
    else:
        ref.v.weight[:] = wt
        ref.v.degree[:] = dg


def env_apply(env, totals, op, i, W, fair, nonrev, per_step):
    m, sp, wt, dg = op_inputs(W, fair, i)
    if op[0] in ("roll", "steps"):
        apply(env, totals, op, nonrev, per_step)
    elif op[0] == "reset_mask":
        env.reset(mask=torch.from_numpy(m))
    elif op[0] == "reset_pos":
        env.reset(mask=torch.from_numpy(m), start_pos=torch.from_numpy(sp))
    else:
        env.set_weight_degree(torch.from_numpy(wt), torch.from_numpy(dg))


def restarts(ref):
    """Per launch: [N] restarts inside it."""
    return [hit.sum(0).astype(np.int64) for _, hit in ref.launches]


def consecutive(ref):
    """How often an env restarted in two consecutive steps of one launch."""
    return sum(int((hit[1:] & hit[:-1]).sum()) for _, hit in ref.launches)


def make(tv, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    return env, new_totals()


def run_sequence(T, W, fair, nonrev, ops):
    tv, oracle = T
    ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
    env, totals = make(tv, W, fair)
    twin, ttot = make(tv, W, fair)
    for i, op in enumerate(ops):
        tag = (W, fair, nonrev, i, op)
        ref_apply(ref, op, i, nonrev)
        env_apply(env, totals, op, i, W, fair, nonrev, False)
        env_apply(twin, ttot, op, i, W, fair, nonrev, True)
        got = pull(env, totals)
        check_against_oracle(got, ref, tag)
        check_against_twin(got, pull(twin, ttot), tag + ("twin",))
    # rs4.nstart / rs4.nenvp of every env: per-step launches with uniform actions until every env has restarted again
    seen = ref.v.episode.copy()
    for j in range(FOLLOW_MAX):
        if (ref.v.episode != seen).all():
            break
        ref.step(count=False)
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
    assert sum(int(r.sum()) for r in restarts(ref)) > N           # games ended and restarted inside the launches


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W,fair", [(4, False), (4, True), (10, True), (24, False), (30, False)])
def test_rollouts_between_the_other_writers(T, W, fair, nonrev):
    """Rollouts after per-step k_obs steps, after tron_reset with an env mask, after tron_reset with start_pos and after
    tron_set_weight_degree (what it puts into rs4.envp stays until the env's first restart, then the launch's own draw)."""
    run_sequence(T, W, fair, nonrev, MIXED)


def oracle_only(oracle, W, fair, nonrev, ops):
    ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
    for i, op in enumerate(ops):
        ref_apply(ref, op, i, nonrev)
    return ref


@pytest.mark.parametrize("ops", [ROLLS, MIXED], ids=["rolls", "mixed"])
def test_inputs_reach_the_cases(T, ops):
    """Conditions on the oracle alone (no GPU result enters): the sequences above reach what they are there to reach."""
    _, oracle = T
    for W in (4, 24):
        ref = oracle_only(oracle, W, False, False, ops)
        r = np.concatenate(restarts(ref))
        assert (r == 0).sum() > 0 and (r == 1).sum() > 0 and (r == 2).sum() > 0 and (r >= 3).sum() > 0
        assert consecutive(ref) > 0                               # an env restarts in two consecutive steps of one launch
    for fair in (False, True):                                   # clashing starts: side 4, and `fair`
        inside, at_end = oracle_only(oracle, 4, fair, False, ops).clashes()
        assert inside > 0 and at_end > 0
    # a launch of one step holds envs with no restart and envs with one; set_weight_degree's values must survive in the former
    ref = oracle_only(oracle, 24, False, False, ops)
    one = [hit.sum(0) for _, hit in ref.launches if len(hit) == 1]
    assert one and all((x == 0).any() and (x == 1).any() for x in one)
