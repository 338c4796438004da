"""The step loop of the roll_resident family moves in CELL SPACE.

The loop carries the two heads as indices into the padded board and no r / c: an action's cell delta comes from one
launch-uniform word, collide is the target test alone (off the board is a border WALL), settle's head-on is "the same
cell", and the epilogue divides r and c back out of the cells once — a dead player's head on the border ring must give the
-1 / W it always gave.  A block's action bytes are waited for once, in front of its steps, so a step's tail no longer
drains the lane's LDS queue: a restart's writes and its start-ring read stay in flight into the next step.  (A restart that
leaves the board alone and owes its head chunks until the next written move was built, measured and taken out again:
DESIGN.md, round 21; the cases it needed — first moves behind a restart, a restart in a launch's last step — stay here.)

Everything a caller can read back — both planes, the board, every field of state(), the next-game words (seen after each
env's next restart: the follow-up steps of run_sequence), the totals and, for the record kernel, the three tapes — is
compared exactly with the C oracle and with a twin VecTron that makes every step a launch of its own.  The sequences, the
comparisons and the per-step twin are test_gpu_rollout_entry_masks's run_sequence (built on rollout_support); this file adds
the shapes and step counts the cell-space loop can go wrong at:

Shapes.  Sides 4 (3 chunks, the last one short) and 6 (4 whole chunks, a padded row is one dword): heads that share a chunk
and a dword, deaths on every border in a handful of steps, a restart in nearly every step, envs that die on the first
move behind a restart, twice in a row; 24 (the headline; short last chunk) and 30 (64 chunks: bit 63, S = 32: the delta byte -S = -32); envs 1, 63, 64, 257 and 16 385; `fair` on sides 4 and 6
(start boxes that meet in the middle: both start heads in one dword, first moves into the opponent's start cell).
Step counts.  Consecutive calls of 1, 2, 7, 8, 9, 64, 65 and 72 steps for all three instantiations (k_obs_roll, k_obs_roll_tape,
k_obs_roll_tape_rec) and both policies: launches that end inside a block, on a block's last step and one step behind it, so
that the epilogue packs lanes that restarted in the launch's last step and lanes that have moved since.
Invalidating calls.  entry_masks' INVALIDATE: every call that clears the host's flags between two rollouts, a masked reset, a
per-step step and set_weight_degree among them, and steps without autoreset, behind which the launch is entered with
finished envs (they restart in step 0 without a move).
A launch WITHOUT autoreset has no caller: every rollout entry point of the library sets the flag, so that branch cannot be
reached from a test.

tests/test_rollout_cell_space_cpu.py asserts on the oracle alone that these inputs reach each new path.
"""
import pytest

import test_gpu_rollout_entry_masks as em

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LENS = (1, 2, 7, 8, 9, 64, 65, 72)
SHAPES = [(4, 1, False), (4, 63, True), (4, 257, False), (6, 64, True), (6, 257, False), (6, 63, False), (24, 64, False),
          (24, 257, False), (30, 1, False), (30, 63, False), (30, 257, False)]
LARGE = 16384 + 1
KINDS = {"random": "roll", "tape": "tape", "records": "rec"}


@pytest.fixture(scope="module")
def T():
    tv, oracle = em.gpu_modules(threads=True)
    yield tv, oracle
    em.restore_threads(oracle)


def calls(kind, lens=LENS):
    return [(KINDS[kind], k) for k in lens]


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W,N,fair", SHAPES)
def test_consecutive_rollouts(T, W, N, fair, nonrev):
    em.run_sequence(T, N, W, fair, nonrev, calls("random"))


@pytest.mark.parametrize("kind", ["tape", "records"])
@pytest.mark.parametrize("W,N,fair", SHAPES)
def test_consecutive_tapes(T, W, N, fair, kind):
    em.run_sequence(T, N, W, fair, False, calls(kind))


@pytest.mark.parametrize("kind", ["random", "tape", "records"])
@pytest.mark.parametrize("W", (6, 24))
def test_full_workgroups(T, W, kind):
    """16 385 envs: several game waves per workgroup, the last workgroup with waves that have no env."""
    em.run_sequence(T, LARGE, W, False, kind == "random", calls(kind, (9, 64, 65)))


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W,N,fair", [(4, 257, True), (6, 63, True), (24, 257, False), (30, 64, False)])
def test_every_invalidating_call(T, W, N, fair, nonrev):
    c = em.counts(em.run_sequence(T, N, W, fair, nonrev, em.INVALIDATE))
    assert c["finished"] > 0                                         # (the oracle alone) a launch was entered with finished envs


@pytest.mark.parametrize("W,N,fair", [(4, 63, True), (6, 257, False), (24, 64, False)])
def test_instantiations_interleaved(T, W, N, fair):
    em.run_sequence(T, N, W, fair, False, em.MIXED)
