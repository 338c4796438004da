"""One persistent launch per call.  A call of the roll_resident family (tron_rollout_random, tron_rollout_actions and
tron_rollout_actions_records on the attached int8 codes, mode None: k_obs_roll, k_obs_roll_tape, k_obs_roll_tape_rec) runs
as ONE launch for up to 1 024 steps (ROLL_LAUNCH_CAP), a longer one as launches of 1 024 with the remainder last, where it
ran as launches of 64.  Nothing a caller can read may depend on where the launches split.

What every call leaves behind must be, bit for bit, what the CPU oracle holds after the same steps and what a twin VecTron
holds whose launches are the old ones (TRON_ROLL_CHUNK=64): both observation planes, the board, every field of
VecTron.state() (pos, alive, dir, done, winner, weight, degree, counters), the totals and, where a call records, the three
record tapes.  The library reads TRON_ROLL_CHUNK once per process, so the twin lives in ONE child process for the whole
module (as the twin of tests/test_gpu_rollout_handoff.py does): it runs every case of this file and writes, per case and op,
the SHA-256 of each field's bytes; a case here compares its own fields' digests with them (equal digests of equal-length
byte strings: exact), and every element with the oracle.  rs4's next-game words and the hand-off blob show through what
follows them: every sequence ends with per-step launches until every env has restarted again, and most put a second and
a third long launch behind the first, which enter by its entry masks and its hand-off.

The cases are rollout_long_support.CASES (the oracle's side of them, and that they reach what they are there for:
tests/test_rollout_long_launch_cpu.py).  Steps per call: 65, 72, 127, 128, 129, 136, 255, 256, 257, 320, 1 024, 1 025 and
1 032 — past the old boundary, around both tally flushes, at the cap, one step and one block past it — at sides 4 (fair), 24
and 30 with 257 envs, one call per instantiation and policy.  Envs 1, 64, 65 (257 above) at sides 4 and 24 with `fair` off
and on and at side 30; 16 385 envs (four game waves per workgroup, three at side 30) at sides 4, 24 (fair) and 30.
Sequences: long -> long -> long; long -> per-step launches -> long (the full-read entry); a 200-row tape launch -> a random
rollout; a 200-row tape split 130 + 70 with records; a launch entered with finished envs; a 200-row tape of surviving moves
(envs that do not restart for 64 steps and more) -> a random rollout.
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

from rollout_long_support import CASES, ENVS, FOLLOW_MAX, RANK, SEED, SIDES, STEPS, Model, op_tape
from rollout_support import check_against_oracle, gpu_modules, new_totals, pull, restore_threads

pytestmark = pytest.mark.gpu


def digests(got, rec):
    out = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(got.items())}
    if rec is not None:
        for name, a in zip(("rec_done", "rec_winner", "rec_reward"), rec):
            out[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


def gpu_op(env, totals, op, tape):
    """One op on a VecTron; the record tapes (done, winner, reward) of a recording op on the host, else None."""
    import torch
    if op[0] == "roll":
        env.rollout_random(op[1], totals, nonreversing=op[2])
    elif op[0] in ("tape", "survive"):
        env.rollout_actions(tape, totals)
    elif op[0] in ("rec", "rec_rows"):
        reward, done, winner = env.rollout_actions(tape, totals, records=True)
        torch.cuda.synchronize()
        return done.cpu().numpy(), winner.cpu().numpy(), reward.cpu().numpy()
    else:
        for _ in range(op[1]):
            env.step(autoreset=op[0] == "steps")
    return None


def gpu_sequence(tv, oracle, name, after_op):
    """The case's ops on one VecTron, then the per-step tail; after_op(i or "follow-j", op, pull()'s dict, record tapes)."""
    import torch
    N, W, fair, ops = CASES[name]
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    totals = new_totals()
    for i, op in enumerate(ops):
        rows = op_tape(N, op, i, oracle, W, fair)
        tape = None if rows is None else torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        rec = gpu_op(env, totals, op, tape)
        after_op(i, op, pull(env, totals), rec)
    j = 0
    while after_op(f"follow-{j}", None, None, None):                 # (the caller says when every env has restarted again)
        env.step()
        after_op(f"followed-{j}", None, pull(env, totals), None)
        j += 1
    env.close()


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


@pytest.fixture(scope="module")
def twin(T, tmp_path_factory):
    """Every case of this file in one child process under TRON_ROLL_CHUNK=64: {case: {op tag: {field: digest}}}."""
    path = str(tmp_path_factory.mktemp("long_launch") / "twin.json")
    env = dict(os.environ, TRON_ROLL_CHUNK="64")
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=600)
    with open(path) as f:
        return json.load(f)


def run_case(T, twin, name):
    tv, oracle = T
    N, W, fair, ops = CASES[name]
    mod = Model(oracle, N, W, fair)
    want = twin[name]
    seen = {}

    def after_op(i, op, got, rec):
        ref = mod.ref
        if got is None:                                              # the tail: go on while some env has not restarted
            if "ep" not in seen:
                seen["ep"] = ref.v.episode.copy()
            more = not (ref.v.episode != seen["ep"]).all()
            if more:
                assert int(i.split("-")[1]) < FOLLOW_MAX
                ref.step(count=False)
            return more
        tag = (name, i, op)
        rows = mod.op(op, i) if op is not None else None
        check_against_oracle(got, ref, tag)
        if rec is not None:
            for field, g_, w_ in zip(("done", "winner", "reward"), rec, rows):
                w_ = w_.astype(g_.dtype)
                assert g_.shape == w_.shape and np.array_equal(g_.view(np.uint8), w_.view(np.uint8)), (tag, field, "oracle")
        assert digests(got, rec) == want.get(str(i)), (tag, "twin")
        return False

    gpu_sequence(tv, oracle, name, after_op)
    assert "ep" in seen and len(want) > len(ops)                     # the tail ran, here and in the twin
    return mod


@pytest.mark.parametrize("W", SIDES)
@pytest.mark.parametrize("K", STEPS)
def test_steps_per_call_every_kernel(T, twin, K, W):
    mod = run_case(T, twin, f"steps-{K}-{W}")
    assert [l["k"] for l in mod.launches] == ([K] if K <= 1024 else [1024, K - 1024]) * 4
    assert [l["handed"] for l in mod.launches][1:] == [True] * (len(mod.launches) - 1)


@pytest.mark.parametrize("W,fair", [(4, False), (4, True), (24, False), (24, True), (30, False)])
@pytest.mark.parametrize("N", ENVS[:3])
def test_one_game_wave_per_workgroup(T, twin, N, W, fair):
    run_case(T, twin, f"envs-{N}-{W}-{int(fair)}")


@pytest.mark.parametrize("W,fair", [(4, False), (24, True), (30, False)])
def test_several_game_waves_per_workgroup(T, twin, W, fair):
    run_case(T, twin, f"envs-{ENVS[4]}-{W}-{int(fair)}")


@pytest.mark.parametrize("N", (65, 257))
@pytest.mark.parametrize("W", SIDES)
@pytest.mark.parametrize("seq", ("long_long", "full_read", "tape_roll", "split_records", "finished"))
def test_sequences(T, twin, seq, W, N):
    mod = run_case(T, twin, f"{seq}-{W}-{N}")
    handed = [l["handed"] for l in mod.launches]
    assert handed == {"long_long": [False, True, True], "full_read": [False, False], "tape_roll": [False, True],
                      "split_records": [False, True], "finished": [False, True]}[seq]
    if seq == "finished":
        assert mod.launches[0]["hit"][0].sum() > mod.launches[0]["fin"][0].sum()   # (the oracle alone) restarts without a move in step 0


@pytest.mark.parametrize("N", (65, 257))
def test_envs_that_do_not_restart(T, twin, N):
    run_case(T, twin, f"idle-30-{N}")


def twin_main(path):
    """The child process: every case, the digests of what each op left (the oracle only makes survive_tape's rows)."""
    import torch
    import oracle
    import tron.vec as tv
    assert torch.cuda.is_available() and os.environ.get("TRON_ROLL_CHUNK") == "64"
    out = {}
    for name in CASES:
        seq = out[name] = {}
        ep = {}

        def after_op(i, op, got, rec):
            if got is None:                                          # the tail: while some env has not restarted, by its own counters
                ep.setdefault("first", ep["now"])
                return not (ep["now"] != ep["first"]).all() and int(i.split("-")[1]) < FOLLOW_MAX
            ep["now"] = got["counters"][:, 1].copy()
            seq[str(i)] = digests(got, rec)
            return False

        gpu_sequence(tv, oracle, name, after_op)
    with open(path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    twin_main(sys.argv[1])
