"""k_obs_roll's helper wave tops its start ring up.  Per env it remembers the highest restart ordinal it has drawn and, behind
every block barrier, draws only up to what the next block can consume: what the block before consumed, not R = 8 ordinals
anew.  In front of the prologue's barrier it draws block 0 alone (its actions, ordinals 1..R); block 1's actions and starts
are drawn during block 0, and the last block's starts stop at what its steps can consume.  What tron_rollout_random leaves
behind must still be, bit for bit, what the CPU oracle stepped the same number of times holds and what a twin VecTron run
with one launch per step (per_step_launches=True: k_obs) holds: both observation planes, the board, every field
VecTron.state() shows (pos, alive, dir, done, winner, weight, degree, counters) and the totals, after every call.  rs4's
next-game words (nstart, nenvp) show as pos / weight / degree after the env's next restart, so every sequence ends with
per-step launches until every env has restarted again, compared with the oracle after each of them.

A sequence is one call per step count, one after the other: 1, 7, 8, 9 (block 1 is one step, its actions drawn during block
0), 15, 16, 17 (the first top-up that is not the full R), 24, 25, 63, 64, 65 and 130 (a new launch primes the helper's
highest ordinal from a new episode).
Envs: 1, 39, 40, 41, 63, 64, 65, 130, 257 (one game wave and one helper per workgroup, ragged last waves); 16 384 + 1 and
16 384 + 200 (four game waves and four helpers per workgroup).  39 / 40 / 41 stand where a split of the prologue's plane
reads between the two roles would fall (SPLIT: the game wave the lower envs, the helper the upper ones); that split is not
built, the shapes are kept as ragged one-wave shapes on both sides of it.  Sides 4 (a restart nearly every step, up to R in
a block, clashing starts), 10, 24 (the workload), 30 (64 chunks, three game waves); `fair` on sides 4 and 10; both action
policies.  One more sequence enters its launches with finished envs (steps without autoreset in front: ordinal 1 is then
consumed in step 0), and one begins its launches with trails in memory (per-step launches in front of the first rollout).

test_inputs_reach_the_cases asserts, from the oracle alone, that these inputs reach the cases they are there for.
"""
import numpy as np
import pytest

from rollout_support import Ref, apply, check_against_oracle, check_against_twin, gpu_modules, new_totals, pull, \
    restore_threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R = 8                                                            # steps per block of the helper (ROLL_R)
SPLIT = 40                                                       # see the docstring
STEPS = (1, 7, 8, 9, 15, 16, 17, 24, 25, 63, 64, 65, 130)
SMALL = (1, SPLIT - 1, SPLIT, SPLIT + 1, 63, 64, 65, 130, 257)
LARGE = (16384 + 1, 16384 + 200)
CASES = [(4, False), (10, False), (24, False), (30, False), (4, True), (10, True)]
LARGE_CASES = [(24, False), (30, False), (4, True)]
SEED, RANK = 0x70B0, 2
FOLLOW_MAX = 64                                                  # per-step launches after a sequence, at the most
ROLLS = [("roll", k) for k in STEPS]
FINISHED = [("steps_noreset", 5), ("roll", 2 * R + 1), ("steps_noreset", 3), ("roll", 65), ("steps_noreset", 2), ("roll", 1),
            ("roll", R + 1)]
TRAILS = [("steps", 6), ("roll", 9), ("steps", 3), ("roll", 17), ("roll", 65)]


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


def mask_chunks(ref):
    """Per env the 16-cell chunks of the player-1 plane that are not the fresh board's (border -1, inside 1): logged at
    every launch's entry (Ref.launch_notes)."""
    p1 = ref.oracle.state_for_player(ref.v.grid, 1).reshape(ref.N, -1)
    fresh = np.where(p1 == -1, -1, 1)
    diff = p1 != fresh
    pad = (-diff.shape[1]) % 16
    diff = np.pad(diff, ((0, 0), (0, pad)))
    return diff.reshape(ref.N, -1, 16).any(2).sum(1)


def consumed(hit):
    """[blocks, N]: the restarts of every env in every block of R steps of one launch (the last block may be partial)."""
    return np.stack([hit[b:b + R].sum(0) for b in range(0, len(hit), R)], 0)


def topups(hit):
    """[blocks - 1, N]: what the helper draws per env during block b for block b + 1, as roll_helper's comment states it:
    hi = len_0 at P; during block b it draws (hi, c_b + R + len_(b+1)]."""
    k = len(hit)
    cons = consumed(hit)
    nb = len(cons)
    hi = np.full(hit.shape[1], min(R, k), np.int64)
    c = np.zeros(hit.shape[1], np.int64)
    out = []
    for b in range(nb - 1):
        to = c + R + min(R, k - (b + 1) * R)
        out.append(np.maximum(to - hi, 0))
        hi = np.maximum(hi, to)
        c = c + cons[b]
    return np.stack(out, 0) if out else np.zeros((0, hit.shape[1]), np.int64)


def make(tv, N, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    return env, new_totals()


def run_sequence(T, N, W, fair, nonrev, ops):
    tv, oracle = T
    ref = Ref(oracle, N, W, SEED, RANK, fair=fair, at_launch=mask_chunks)
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
    assert sum(int(hit.sum()) for _, hit in ref.launches) > N  # games ended and restarted inside the launches


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


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W,fair", [(4, False), (24, False), (30, False)])
def test_launches_begin_with_trails_in_memory(T, W, fair, nonrev):
    ref = run_sequence(T, 130, W, fair, nonrev, TRAILS)
    # (the oracle alone) masks of more than two chunks at a launch's entry; a 4x4 game's board is three chunks in all
    assert max(int(chunks.max()) for chunks in ref.launch_notes) > (2 if W > 4 else 1)


def oracle_only(oracle, N, W, fair, nonrev, ops):
    ref = Ref(oracle, N, W, SEED, RANK, fair=fair, at_launch=mask_chunks)
    for op in ops:
        ref.apply(op, nonrev)
    return ref


def reached(oracle):
    """The counts test_inputs_reach_the_cases asserts on, from the oracle alone (no GPU)."""
    out = {}
    ref4 = oracle_only(oracle, 130, 4, False, False, ROLLS)
    ref24 = oracle_only(oracle, 130, 24, False, False, ROLLS)
    # An env with R restarts in one block and none in the next one.  The block with none is a launch's short last block
    # (9, 17, 25 steps: one step; 130 = 64 + 64 + 2): a whole block of R steps without a restart cannot follow at side 4,
    # where a game fills the 16 cells in 7 steps, and on a larger board R restarts in one block do not occur (none in
    # 16 384 envs x 64 steps at 24x24).  Rare even so: the 16 384 + 1 envs of the four-wave shape (side 4, `fair`) reach it.
    ref4l = oracle_only(oracle, LARGE[0], 4, True, False, ROLLS)
    n = 0
    for _, hit in ref4l.launches:
        cons = consumed(hit)
        n += int(((cons[:-1] == R) & (cons[1:] == 0)).sum())
    out["R restarts in a block, then a block with none (side 4, fair, 16 385 envs)"] = n
    # two lanes of one wave whose consumption in one block differs by at least 4
    for name, ref in (("side 4", ref4), ("side 24", ref24)):
        n = 0
        for _, hit in ref.launches:
            cons = consumed(hit)
            for w0 in range(0, 130, 64):
                cw = cons[:, w0:w0 + 64]
                n += int((cw.max(1) - cw.min(1) >= 4).sum())
        out[f"wave-blocks whose lanes' consumption differs by >= 4 ({name})"] = n
    # top-ups past block 0 (drawn during block b >= 1) of 0 and of R
    for name, ref in (("side 4", ref4), ("side 24", ref24)):
        t = [topups(hit)[1:] for _, hit in ref.launches if len(hit) > 2 * R]
        out[f"top-ups of 0 past block 0 ({name})"] = sum(int((x == 0).sum()) for x in t)
        if ref is ref4:                                          # (at 24x24 no env restarts R times in one block)
            out[f"top-ups of R past block 0 ({name})"] = sum(int((x == R).sum()) for x in t)
        out[f"partial top-ups past block 0, 1..R-1 ({name})"] = sum(int(((x > 0) & (x < R)).sum()) for x in t)
    for fair in (False, True):
        ref = ref4 if not fair else oracle_only(oracle, 130, 4, True, False, ROLLS)
        out[f"clashing starts among the first 16 envs (side 4, fair={fair})"] = ref.clashes()[0]
    # an env of the upper lanes of a wave (SPLIT and above) whose mask at launch entry has more than two chunks
    for name, ref in (("side 24, rollouts only", ref24), ("side 24, per-step launches first", oracle_only(oracle, 130, 24, False, False, TRAILS))):
        upper = (np.arange(130) % 64) >= SPLIT
        out[f"env-launches of the upper lanes entered with more than two chunks in the mask ({name})"] = \
            sum(int((chunks[upper] > 2).sum()) for chunks in ref.launch_notes)
    out["env-launches entered finished (side 24)"] = oracle_only(oracle, 130, 24, False, False, FINISHED).entered_done
    return out


def test_inputs_reach_the_cases(T):
    """Conditions on the oracle alone (no GPU result enters): the sequences above reach what they are there to reach."""
    _, oracle = T
    out = reached(oracle)
    for k, v in out.items():
        print(f"{k}: {v}")
    for k, v in out.items():
        assert v > 0, k
