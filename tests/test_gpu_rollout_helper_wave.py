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
import numpy as np
import pytest

from rollout_support import Ref, apply, check_against_oracle, check_against_twin, gpu_modules, new_totals, pull, \
    restore_threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R = 8                                                            # steps per block of the helper (ROLL_R)
STEPS = (1, R - 1, R, R + 1, 2 * R, 2 * R + 1, 63, 64, 65, 130)
SMALL = (1, 63, 64, 65, 130, 257)
LARGE = (16384 + 1, 16384 + 200)
CASES = [(4, False), (10, False), (24, False), (30, False), (4, True), (10, True)]
LARGE_CASES = [(24, False), (30, False), (4, True)]
SEED, RANK = 0xB10C, 1
FOLLOW_MAX = 64                                                  # per-step launches after a sequence, at the most
ROLLS = [("roll", k) for k in STEPS]
FINISHED = [("steps_noreset", 5), ("roll", 2 * R + 1), ("steps_noreset", 3), ("roll", 65), ("steps_noreset", 2), ("roll", 1),
            ("roll", R)]


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


def make(tv, N, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    return env, new_totals()


def run_sequence(T, N, W, fair, nonrev, ops):
    tv, oracle = T
    ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
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
        ref.step(count=False)
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
    ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
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
        assert oracle_only(oracle, 130, 4, fair, False, ROLLS).clashes()[0] > 0
    ref = oracle_only(oracle, 130, 24, False, False, FINISHED)
    assert ref.entered_done > 0                                  # envs that are finished when a launch begins
