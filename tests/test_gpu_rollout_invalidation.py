"""Every entry point that writes the attached planes or the state words, between two persistent rollouts.  A launch of the
roll_resident family leaves entry masks and a hand-off for the next one; the host drops both when any other kernel that can
write the planes or st4 / rs4 is enqueued (the launcher does it, by the kernel's row in writes_state), and the next
rollout must then read whole planes and draw its own first block.

One case per writer: a 3-step tron_rollout_random on the attached codes (mode None), the writer, another 3-step rollout.
After each of the three phases both observation planes, the board, every field of VecTron.state() and the totals must equal
the CPU oracle's, bit for bit.  The writers: tron_reset with a partial mask, tron_step_encode, tron_step_encode with
TRON_STEP_INCREMENTAL, both parts of tron_step_encode_part, tron_set_weight_degree, tron_attach_obs_state of a second buffer
(refused: the buffer stays), tron_rollout_random with TRON_ROLLOUT_PER_STEP and with TRON_ROLLOUT_TWO_STREAMS,
tron_rollout_actions with TRON_ROLLOUT_PER_STEP.

Shape: 130 envs (two full waves and a ragged third) on a 6x6 board (side 8, G = 64, four chunks): more than one wave, a
ragged tail, and games short enough that envs restart within the six rollout steps (asserted on the oracle alone).

The ops and their oracle side are test_gpu_rollout_entry_masks.py's (gpu_op, model_op, Model), which runs most of these
writers in longer sequences at larger shapes; the two-stream rollout is the one op it has no name for.
"""
import pytest

import test_gpu_rollout_entry_masks as em
from rollout_support import check_against_oracle, gpu_modules, make_tape, pull

pytestmark = pytest.mark.gpu

N, W, K = 130, 6, 3
# name -> (op of test_gpu_rollout_entry_masks.gpu_op / model_op, its per_step argument)
WRITERS = {
    "reset_mask": (("reset_mask",), False),
    "step": (("steps", 1), False),
    "step_incremental": (("inc",), False),
    "step_parts": (("part",), False),
    "set_weight_degree": (("wd",), False),
    "attach_other": (("attach_other",), False),
    "rollout_per_step": (("roll", K), True),
    "rollout_two_streams": (("roll", K), None),
    "actions_per_step": (("tape", K), True),
}


@pytest.fixture(scope="module")
def T():
    return gpu_modules()


@pytest.mark.parametrize("writer", list(WRITERS))
def test_writer_between_rollouts(T, writer):
    tv, oracle = T
    mod = em.Model(oracle, N, W, False)
    env, totals = em.make(tv, N, W, False)

    def phase(i, op, per_step):
        tape = make_tape(N, op[1], salt=i) if op[0] == "tape" else None
        if per_step is None:
            env.rollout_random(op[1], totals, two_streams=True)
        else:
            em.gpu_op(tv, env, totals, op, i, False, per_step, tape)
        em.model_op(mod, op, i, False, None if tape is None else tape.cpu().numpy())
        check_against_oracle(pull(env, totals), mod.ref, (writer, i, op))

    phase(0, ("roll", K), False)
    phase(1, *WRITERS[writer])
    phase(2, ("roll", K), False)
    assert sum(mod.ref.restarts_per_step) > 0                       # (the oracle alone) envs restarted within the steps
    env.close()
