"""The one step body of the roll_resident family (k_obs_roll, k_obs_roll_tape, k_obs_roll_tape_rec).

A step has one LDS round trip and one piece of board code: the move's reads (the two new heads' dwords, the template's
chunks of theirs) go out together with the next game's kit (the template's dwords of the two start chunks, the start ring's
word of the game after it), the move is judged, and the board work — refresh a chunk from the template, set the head
nibbles, mark the chunks — runs once, at the new heads for a move that goes on and at the start cells for a restart (in the
step the game finishes in, or in a launch's first step for an env that entered finished).  A restart's tail waits for nothing.

Everything a caller can read back — both planes, the board, every field of state(), the totals, the three record tapes
under DQN's reward table, and rs4's next-game words (seen after each env's next restart: the per-step tail) — is compared
exactly with the C oracle, with a twin VecTron that makes every step a launch of its own, and with a twin in a child process
whose launches all draw their own first block (TRON_ROLL_NO_HANDOFF; the library reads it once per process, so one child
runs every case and returns digests).

The sequence and the shapes are rollout_short_chain_support's under another seed and stream (rollout_one_body_support): per
k of 1, 2, 7, 8, 9, 20, 129 a reset and three calls of k steps (a full-read entry, then two masked, handed entries), then
calls behind per-step steps with and without autoreset, then a reset and a launch whose tape's first row is safe for every env
(a whole wave on the move path, no lane restarting) with a handed tape call behind it; sides 4, 6, 24, 30; 1, 65 and 257 envs; the uniform and the
non-reversing policy, a tape, a tape with records; `fair` off and on.

tests/test_rollout_one_body_cpu.py asserts on the oracle alone that these inputs contain the cases the body can break.
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

from rollout_one_body_support import FOLLOW_MAX, KINDS, NS, OPS, RANK, SEED, SIDES, Model, host_tape, safe_tape
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
    elif kind in ("uniform", "nonreversing") and op[0] == "call":
        env.rollout_random(op[1], totals, nonreversing=kind == "nonreversing", per_step_launches=per_step)
    elif kind != "records":                                            # (the safe tape is played by every kind)
        env.rollout_actions(tape, totals, per_step_launches=per_step)
    else:
        reward, done, winner = env.rollout_actions(tape, totals, per_step_launches=per_step, records=True)
        torch.cuda.synchronize()
        return done.cpu().numpy(), winner.cpu().numpy(), reward.cpu().numpy()
    return None


def op_tape(env, W, op, i, kind):
    """The tape of a call on the device: make_tape's, or, for the op "safe", safe_tape from the heads the env reports."""
    import torch
    if op[0] == "safe":
        return torch.from_numpy(safe_tape(pull(env)["pos"], W, op[1], salt=i)).cuda()
    return make_tape(env.N, op[1], salt=i) if op[0] == "call" and kind in ("tape", "records") else None


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
    path = str(tmp_path_factory.mktemp("one_body") / "drawn.json")
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, TRON_ROLL_NO_HANDOFF="1"), check=True,
                   timeout=600)
    with open(path) as f:
        return json.load(f)


@pytest.mark.parametrize("W,N,fair,kind", CASES)
def test_one_body(T, drawn, W, N, fair, kind):
    tv, oracle = T
    mod = Model(oracle, N, W, fair, kind)
    want = drawn[case_name(W, N, fair, kind)]
    env, totals = make(tv, N, W, fair)
    twin, ttot = make(tv, N, W, fair)
    for i, op in enumerate(OPS):
        tag = (W, N, fair, kind, i, op)
        tape = op_tape(env, W, op, i, kind)
        host = None if tape is None else tape.cpu().numpy()
        want_tape = safe_tape(mod.ref.v.pos, W, op[1], salt=i) if op[0] == "safe" else None if host is None else host_tape(N, op[1], salt=i)
        assert host is None or np.array_equal(host, want_tape)      # (what the CPU file counts on)
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
            rec = gpu_op(env, totals, op, kind, op_tape(env, W, op, i, kind))
            seq[str(i)] = digests(pull(env, totals), rec)
        env.close()
    with open(path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    twin_main(sys.argv[1])
