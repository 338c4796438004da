"""k_obs_roll no longer wipes a finished game's trail when the env restarts: the trail's chunks go `stale` (their bytes in
LDS are garbage, their content is the fresh-board template), a move refreshes the chunk of a new head only when it steps into
one, and the launch's epilogue stores a stale chunk from the template.  What
tron_rollout_random leaves behind must still be, bit for bit, what the CPU oracle stepped the same number of times holds and
what a twin VecTron run with one launch per step (per_step_launches=True: k_obs) holds: the whole [N, 2, G] observation
buffer, the board, every field VecTron.state() shows and the totals.

Shapes are the smallest at which the new paths can go wrong.  Widths: 4 (G = 36: a short last chunk that goes stale, restarts
nearly every step, more than half of a wave restarting at once), 10 (whole chunks only), 24 (the workload's chunking, short
chunk of 4), 30 (64 chunks: bit 63 of `stale`, three waves per workgroup).  Envs: 1, 63, 130 (a partly filled third wave),
257 (a second workgroup with one env).  Steps: 1, 2, 63, 64, 65 (the launch split at 64), 130 (three launches: the second and
third prologue rebuild the masks from what an epilogue with stale chunks wrote).  Both action distributions; `fair` start
placement (three Philox blocks per restart, clashing starts common) at widths 4 and 10, oracle and twin created alike.

test_inputs_reach_the_rare_paths asserts, on the oracle alone, that these inputs do reach the paths they are there for.
"""
import numpy as np
import pytest

from rollout_support import LAUNCH, Ref, check_against_oracle, check_against_twin, gpu_modules, new_totals, pull, restore_threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = (4, 10, 24, 30)
FAIR_WIDTHS = (4, 10)
ENVS = (1, 63, 130, 257)
STEPS = (1, 2, 63, 64, 65, 130)
SEED, RANK = 0xC0FFEE, 2
CASES = [(W, False) for W in WIDTHS] + [(W, True) for W in FAIR_WIDTHS]


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


_REFS = {}


def reference(oracle, N, W, nonrev, fair):
    """The oracle's snapshots after each step count of STEPS: computed once per case, never modified."""
    key = (N, W, nonrev, fair)
    if key not in _REFS:
        ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
        snaps = {}
        for k in range(1, max(STEPS) + 1):
            ref.step(nonrev=nonrev)
            if k in STEPS:
                snaps[k] = ref.snapshot()
        _REFS[key] = snaps
    return _REFS[key]


def make(tv, N, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    return env, new_totals()


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N", ENVS)
@pytest.mark.parametrize("W,fair", CASES)
def test_lazy_rebuild_equals_oracle_and_per_step_twin(T, W, fair, N, nonrev):
    """The oracle and the per-step twin, after every step count of STEPS from a fresh reset."""
    tv, oracle = T
    snaps = reference(oracle, N, W, nonrev, fair)
    for K in STEPS:
        env, totals = make(tv, N, W, fair)
        env.rollout_random(K, totals, nonreversing=nonrev)
        got = pull(env, totals)
        check_against_oracle(got, snaps[K], (W, fair, N, nonrev, K))
        twin, ttot = make(tv, N, W, fair)
        twin.rollout_random(K, ttot, nonreversing=nonrev, per_step_launches=True)
        check_against_twin(got, pull(twin, ttot), (W, fair, N, nonrev, K, "twin"))
        env.close()
        twin.close()
    assert int(snaps[max(STEPS)]["episode"].max()) > 3          # games ended and restarted inside the launches


def chunks_off_template(grid, fresh):
    """[N, chunks] bool: the 16-cell chunks of each board that differ from the fresh board."""
    N, G = grid.shape
    cpe = (G + 15) // 16
    d = np.zeros((N, cpe * 16), bool)
    d[:, :G] = grid != fresh
    return d.reshape(N, cpe, 16).any(2)


def head_chunks(pos, S):
    """[N, 2] chunk index of each head (an out-of-bounds head is on the border wall cell)."""
    p = pos.astype(np.int64)
    return np.stack([((p[:, 0] + 1) * S + p[:, 1] + 1) >> 4, ((p[:, 2] + 1) * S + p[:, 3] + 1) >> 4], 1)


def walk(oracle, N, W, fair, steps):
    """Steps the oracle and follows, per env, the chunks the kernel would hold stale: at a restart the chunks that
    differed from the template before the step (less the new heads'), until a later move of the same launch puts a head
    there.  Returns (moves into a stale chunk, envs whose launch ended with a stale chunk that differed from the template
    when the launch began, the largest number of the first 64 envs restarting in one step, the oracle)."""
    ref = oracle.VecOracle(N, W, seed=SEED, stream=RANK, fair=fair)
    ref.reset_all()
    S = W + 2
    fresh = np.zeros((S, S), np.int8)
    fresh[0, :] = fresh[-1, :] = fresh[:, 0] = fresh[:, -1] = -1
    fresh = fresh.reshape(-1)
    rows = np.arange(N)
    stale = np.zeros((N, (S * S + 15) // 16), bool)
    mask0 = chunks_off_template(ref.grid, fresh)
    into_stale = left_stale = most_restarts = 0
    for k in range(1, steps + 1):
        before = chunks_off_template(ref.grid, fresh)
        ep = ref.episode.copy()
        ref.step(autoreset=True, want_obs=False)
        restarted = ref.episode != ep
        most_restarts = max(most_restarts, int(restarted[:64].sum()))
        hc = head_chunks(ref.pos, S)
        moved = ~restarted
        for p in range(2):
            into_stale += int((stale[rows, hc[:, p]] & moved).sum())
        stale[restarted] |= before[restarted]
        for p in range(2):
            stale[rows, hc[:, p]] = False                        # a move refreshes it; a restart writes its head chunks
        if k % LAUNCH == 0 or k == steps:
            left_stale += int((stale & mask0).any(1).sum())
            stale[:] = False
            mask0 = chunks_off_template(ref.grid, fresh)
    return into_stale, left_stale, most_restarts, ref


def test_inputs_reach_the_rare_paths(T):
    """Conditions on the oracle alone (no GPU result enters): the shapes above reach what they are there to reach."""
    _, oracle = T
    into_stale, left_stale, _, _ = walk(oracle, 130, 24, False, 130)
    assert into_stale >= 1          # a head moves into a chunk an earlier episode of the same launch left non-template
    assert left_stale >= 1          # a launch ends with such a chunk never revisited (and in the launch's first mask: stored from the template)
    _, _, most, _ = walk(oracle, 130, 4, False, 130)
    assert most > 32                # more than half of the first wave restarts in one step
    _, _, _, ref = walk(oracle, 130, 4, True, 130)
    clashes = 0
    for e in range(64):
        for ep in range(2, int(ref.episode[e]) + 1):
            words = np.concatenate([oracle.philox([e, ep, 2, b], [SEED, RANK]) for b in range(24)])
            clashes += oracle.make_game(4, True, words)[3] > 9   # nine draws without a clash (point, 4 starts, 2 weights, degree)
    assert clashes >= 1             # a `fair` restart whose two starts clash: the general routine runs
