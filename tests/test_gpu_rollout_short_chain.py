"""The shorter step chain of the roll_resident family (k_obs_roll, k_obs_roll_tape, k_obs_roll_tape_rec).

The start ring and the hand-off words hold a game's two start CELLS (16 + 16 bits), so a restart converts nothing and the
epilogue divides rs4.nstart back out for a lane that restarted; a move marks only its two new head chunks in mask and
dirty (the old heads' chunks are in both already); a restart writes the template's dwords of its head chunks and then sets
the two head nibbles; the launch-uniform policy flag is a template argument of the block's steps.  (Deriving eplen and
tick in the epilogue instead of carrying them was built and taken out again; its cases — restarts in a launch's first and
last step, lanes that enter finished, rewards that depend on eplen — stay here.)

Everything a caller can read back — both planes, the board, every field of state(), the totals, the three record tapes
under DQN's reward table (the step reward is the episode's step index: eplen), and rs4's next-game words (seen after each
env's next restart: the per-step tail) — is compared exactly with the C oracle, with a twin VecTron that makes every step
a launch of its own, and with a twin in a child process whose launches all draw their own first block
(TRON_ROLL_NO_HANDOFF; the library reads it once per process, so one child runs every case and returns digests).

The sequence (rollout_short_chain_support.OPS): per k of 1, 2, 7, 8, 9, 20, 129 a reset and three consecutive calls of k
steps — a full-read entry that draws, then two masked, handed entries; 2 is there for side 4, whose games end within 7
steps, so that some env goes through a launch without a restart —, then calls behind per-step steps with and without
autoreset, which invalidate the hand-off (behind the latter the launch is entered with finished envs).
Sides 4 and 6 (few cells and chunks, both heads often in one dword), 24 (the short last chunk), 30 (64 chunks, mask bit 63);
1, 65 and 257 envs (lanes without an env, a partial last wave); the uniform and the non-reversing policy, a tape, a tape
with records; `fair` on and off (the two-block start draw).

tests/test_rollout_short_chain_cpu.py asserts on the oracle alone that these inputs contain the cases the change can break.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":                                           # the twin process: the paths conftest.py sets up
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "deep-q-learning_tron_amd"), os.path.dirname(os.path.abspath(__file__))]

from rollout_short_chain_support import FOLLOW_MAX, KINDS, NS, OPS, RANK, SEED, SIDES, Model, host_tape
from rollout_support import check_against_oracle, check_against_twin, gpu_modules, make_tape, new_totals, pull, restore_threads

pytestmark = pytest.mark.gpu

CASES = [(W, N, fair, kind) for W in SIDES for N in NS for fair in (False, True) for kind in KINDS]


def case_name(W, N, fair, kind):
    return f"{kind}-{W}-{N}-{int(fair)}"


def make(tv, N, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair, reward="dqn")
    assert env.obs_is_state
    env.reset()
    return env, new_totals()


def gpu_op(env, totals, op, kind, tape, per_step=False):
    """One op on a VecTron; the record tapes of a call with records on the host, else None."""
    import torch
    if op[0] == "reset":
        env.reset()
    elif op[0] in ("steps", "steps_noreset"):
        for _ in range(op[1]):
            env.step(autoreset=op[0] == "steps", nonreversing=kind == "nonreversing")
    elif kind in ("uniform", "nonreversing"):
        env.rollout_random(op[1], totals, nonreversing=kind == "nonreversing", per_step_launches=per_step)
    elif kind == "tape":
        env.rollout_actions(tape, totals, per_step_launches=per_step)
    else:
        reward, done, winner = env.rollout_actions(tape, totals, per_step_launches=per_step, records=True)
        torch.cuda.synchronize()
        return done.cpu().numpy(), winner.cpu().numpy(), reward.cpu().numpy()
    return None


def op_tape(N, op, i, kind):
    return make_tape(N, op[1], salt=i) if op[0] == "call" and kind in ("tape", "records") else None


def digests(got, rec):
    out = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(got.items())}
    if rec is not None:
        for name, a in zip(("rec_done", "rec_winner", "rec_reward"), rec):
            out[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


@pytest.fixture(scope="module")
def drawn(T, tmp_path_factory):
    """Every case in one child process under TRON_ROLL_NO_HANDOFF: {case: {op index: {field: digest}}}."""
    path = str(tmp_path_factory.mktemp("short_chain") / "drawn.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, TRON_ROLL_NO_HANDOFF="1"), check=True,
                   timeout=600)
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("W,N,fair,kind", CASES)
def test_short_chain(T, drawn, W, N, fair, kind):
    tv, oracle = T
    mod = Model(oracle, N, W, fair, kind)
    want = drawn[case_name(W, N, fair, kind)]
    env, totals = make(tv, N, W, fair)
    twin, ttot = make(tv, N, W, fair)
    for i, op in enumerate(OPS):
        tag = (W, N, fair, kind, i, op)
        tape = op_tape(N, op, i, kind)
        host = None if tape is None else tape.cpu().numpy()
        assert host is None or np.array_equal(host, host_tape(N, op[1], salt=i))     # (what the CPU file counts on)
        rows = mod.op(op, host)
        rec = gpu_op(env, totals, op, kind, tape)
        trec = gpu_op(twin, ttot, op, kind, tape, per_step=True)
        got = pull(env, totals)
        check_against_oracle(got, mod.ref, tag)
        check_against_twin(got, pull(twin, ttot), tag + ("per-step twin",))
        if rec is not None:
            for name, g_, t_, w_ in zip(("done", "winner", "reward"), rec, trec, rows):
                assert g_.shape == t_.shape and np.array_equal(g_.view(np.uint8), t_.view(np.uint8)), (tag, name, "per-step twin")
                w_ = w_.astype(g_.dtype)
                assert g_.shape == w_.shape and np.array_equal(g_.view(np.uint8), w_.view(np.uint8)), (tag, name, "oracle")
        assert digests(got, rec) == want[str(i)], (tag, "TRON_ROLL_NO_HANDOFF twin")
    # rs4.nstart / rs4.nenvp of every env: per-step launches with uniform actions until every env has restarted again
    ref = mod.ref
    seen = ref.v.episode.copy()
    for j in range(FOLLOW_MAX):
        if (ref.v.episode != seen).all():
            break
        ref.step(count=False)
        env.step()
        twin.step()
        check_against_oracle(pull(env, totals), ref, (W, N, fair, kind, "follow", j))
    assert (ref.v.episode != seen).all()                             # (the oracle alone) the next game of every env was looked at
    check_against_twin(pull(env, totals), pull(twin, ttot), (W, N, fair, kind, "follow", "per-step twin"))
    env.close()
    twin.close()


def twin_main(path):
    """The child process: every case without an oracle, the digests of what each op left."""
    import torch
    import tron.vec as tv
    assert torch.cuda.is_available() and os.environ.get("TRON_ROLL_NO_HANDOFF")
    out = {}
    for W, N, fair, kind in CASES:
        seq = out[case_name(W, N, fair, kind)] = {}
        env, totals = make(tv, N, W, fair)
        for i, op in enumerate(OPS):
            rec = gpu_op(env, totals, op, kind, op_tape(N, op, i, kind))
            seq[str(i)] = digests(pull(env, totals), rec)
        env.close()
    with open(path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    twin_main(sys.argv[1])
