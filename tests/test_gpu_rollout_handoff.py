"""k_obs_roll's hand-off.  The helper wave of every launch of the roll_resident family (tron_rollout_random,
tron_rollout_actions, tron_rollout_actions_records on the attached int8 codes, mode None) spends its last block on the NEXT
launch: it tops the start ring up, draws the next launch's block-0 action bytes (not behind a tape) and stores ring, bytes and
the ring's level per env.  The next such launch, if no call that can write the state words was enqueued in between, loads these
words instead of drawing 16 Philox blocks per env in front of its first step.  The start ring is keyed by the absolute
episode, so that the image still means something once the episode count has moved on.

What a call leaves behind must be, bit for bit, what the CPU oracle holds after the same steps and what a twin VecTron holds
whose launches all draw their own first block (TRON_ROLL_NO_HANDOFF): both observation planes, the board, every field of
VecTron.state() (pos, alive, dir, done, winner, weight, degree, counters), the totals and, where a call records, the three
record tapes.  The library reads TRON_ROLL_NO_HANDOFF once per process, so the twin lives in ONE child process for the whole
module: it runs every case of this file and writes, per case and op, the SHA-256 of each field's bytes; a case here compares
its own fields' digests with them (equal digests of equal-length byte strings: exact), and every element with the oracle.
rs4's next-game words show as pos / weight / degree after an env's next restart, so every sequence ends with per-step
launches until every env has restarted again.

Shapes.  Sides 4, 10, 24, 30; 1, 63, 130 and 257 envs (one game wave per workgroup, ragged) and 16 385 envs at side 24 (four
game waves per workgroup, the last workgroup with waves that have no env); `fair` on and off.
Sequences.  ROLLS: consecutive calls of 1, 7, 8, 9, 15, 16, 17, 64, 65 and 130 steps, the uniform and the non-reversing
policy alternating: hand-offs from and to launches of one block, short last blocks and the second and third launch of one
call.  MIXED_A / MIXED_B: random, tape and tape-with-records calls interleaved, in both orders: a tape launch hands over
starts alone, and the launch behind it draws its actions (or copies its rows) and takes the starts.  INVALIDATE: between two
rollouts a masked reset, per-step steps, set_weight_degree and a re-attach (which the library refuses before it touches
anything: the buffer stays, and so does the hand-off).  FINISHED: steps without autoreset first, so that the first
launch enters with finished envs (and draws) and hands over to the second.

test_inputs_reach_the_cases asserts on the oracle alone that the inputs reach the cases they are there for.
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

from rollout_support import LAUNCH, Ref, check_against_oracle, gpu_modules, make_tape, new_totals, pull, restore_threads

pytestmark = pytest.mark.gpu

SEED, RANK = 0x4A2D, 5
SIDES = (4, 10, 24, 30)
SMALL = (1, 63, 130, 257)
LARGE = 16384 + 1
R = 8                                                            # steps per block (ROLL_R)
FOLLOW_MAX = 64
# (op, steps, non-reversing policy)
ROLLS = [("roll", k, i % 2 == 1) for i, k in enumerate((1, 7, 8, 9, 15, 16, 17, 64, 65, 130))]
MIXED_A = [("roll", 9, False), ("tape", 9), ("roll", 17, True), ("rec", 65), ("roll", 8, False), ("tape", 130), ("rec", 7),
           ("roll", 65, False)]
MIXED_B = [("tape", 9), ("roll", 9, True), ("rec", 17), ("roll", 65, False), ("tape", 8), ("rec", 130), ("roll", 7, False),
           ("tape", 65)]
INVALIDATE = [("roll", 9, False), ("roll", 9, False), ("reset_mask",), ("roll", 9, False), ("roll", 17, True), ("steps", 2),
              ("roll", 9, False), ("roll", 9, False), ("wd",), ("roll", 9, False), ("roll", 9, False), ("attach_same",),
              ("roll", 9, False), ("roll", 9, False)]
FINISHED = [("steps_noreset", 5), ("roll", 17, False), ("roll", 9, False), ("roll", 65, True)]
LARGE_SEQ = [("roll", 9, False), ("roll", 17, True), ("tape", 9), ("roll", 65, False)]

CASES = {}                                                       # name -> (N, W, fair, ops): what the twin process runs
for _W in SIDES:
    for _N in SMALL:
        for _f in (False, True):
            CASES[f"rolls-{_W}-{_N}-{int(_f)}"] = (_N, _W, _f, ROLLS)
for _W, _f in ((4, True), (10, False), (24, False), (30, True)):
    for _N in (63, 257):
        CASES[f"mixed_a-{_W}-{_N}"] = (_N, _W, _f, MIXED_A)
        CASES[f"mixed_b-{_W}-{_N}"] = (_N, _W, _f, MIXED_B)
        CASES[f"invalidate-{_W}-{_N}"] = (_N, _W, _f, INVALIDATE)
        CASES[f"finished-{_W}-{_N}"] = (_N, _W, _f, FINISHED)
CASES["large-24"] = (LARGE, 24, False, LARGE_SEQ)


def op_inputs(N, W, i):
    """The arguments of the i-th op of a sequence (a masked reset's mask, set_weight_degree's values)."""
    rs = np.random.RandomState(104729 * W + 37 * i + N)
    m = (rs.rand(N) < 0.4).astype(np.int8)
    m[0] = 1
    return m, rs.randint(40, 102, (N, 2)).astype(np.int16), rs.randint(-30, 31, N).astype(np.int16)


def digests(got, rec):
    out = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(got.items())}
    if rec is not None:
        for name, a in zip(("rec_done", "rec_winner", "rec_reward"), rec):
            out[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


def gpu_op(tv, env, totals, op, i, tape):
    """One op on a VecTron; the record tapes of a ("rec", K) op on the host, else None."""
    import torch
    m, wt, dg = op_inputs(env.N, env.W, i)
    if op[0] == "roll":
        env.rollout_random(op[1], totals, nonreversing=op[2])
    elif op[0] == "tape":
        env.rollout_actions(tape, totals)
    elif op[0] == "rec":
        reward, done, winner = env.rollout_actions(tape, totals, records=True)
        torch.cuda.synchronize()
        return done.cpu().numpy(), winner.cpu().numpy(), reward.cpu().numpy()
    elif op[0] == "reset_mask":
        env.reset(mask=torch.from_numpy(m))
    elif op[0] in ("steps", "steps_noreset"):
        for _ in range(op[1]):
            env.step(autoreset=op[0] == "steps")
    elif op[0] == "attach_same":
        with torch.cuda.device(env.device):
            rc = env._lib.tron_attach_obs_state(env._h, tv.nat.ptr(env.obs), tv.nat.stream_ptr())
        assert rc != 0                                               # already attached: refused, the buffer stays
    elif op[0] == "wd":
        env.set_weight_degree(torch.from_numpy(wt), torch.from_numpy(dg))
    else:
        raise ValueError(op)
    return None


def gpu_sequence(tv, N, W, fair, ops, after_op):
    """The ops on one VecTron, then the per-step tail; after_op(i or "follow-j", op, pull()'s dict, record tapes)."""
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    totals = new_totals()
    for i, op in enumerate(ops):
        tape = make_tape(N, op[1], salt=i) if op[0] in ("tape", "rec") else None
        rec = gpu_op(tv, env, totals, op, i, tape)
        after_op(i, op, pull(env, totals), rec, tape)
    j = 0
    while after_op(f"follow-{j}", None, None, None, None):           # (the caller says when every env has restarted again)
        env.step()
        after_op(f"followed-{j}", None, pull(env, totals), None, None)
        j += 1
    env.close()


class Model:
    """The oracle side of a sequence: a Ref, the host's flag as the issue states it (`handed`: the last op was a persistent
    launch with autoreset) and, per launch of the roll_resident family, what it entered with and which envs restarted when."""

    def __init__(self, oracle, N, W, fair):
        self.ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
        self.oracle, self.N, self.W, self.fair = oracle, N, W, fair
        self.handed = False
        self.launches = []                                           # (handed, tape, [N] episode before, [k, N] restarted in step s)

    def rollout(self, K, nonrev=False, tape=None):
        """K steps with autoreset as a rollout call makes them; the (done, winner, reward) rows of every step."""
        rows = []
        v = self.ref.v
        if K < 2:                                                    # a single step is a per-step launch
            self.handed = False
        for k0 in range(0, K, LAUNCH):
            k = min(K, k0 + LAUNCH) - k0
            before = v.episode.copy()
            hit = np.zeros((k, self.N), bool)
            for s in range(k):
                ep = v.episode.copy()
                rows.append(self.ref.step(actions=None if tape is None else tape[k0 + s], nonrev=nonrev))
                hit[s] = v.episode != ep
            if K >= 2:
                self.launches.append((self.handed, tape is not None, before, hit))
                self.handed = True
        return tuple(np.stack([r[i] for r in rows]) for i in range(3))

    def op(self, op, i, tape):
        v = self.ref.v
        m, wt, dg = op_inputs(self.N, self.W, i)
        if op[0] in ("roll", "tape", "rec"):
            return self.rollout(op[1], op[2] if op[0] == "roll" else False, tape)
        if op[0] != "attach_same":                                   # (refused: nothing is written, nothing is cleared)
            self.handed = False
        if op[0] == "reset_mask":
            v.reset_masked(m)
        elif op[0] in ("steps", "steps_noreset"):
            for _ in range(op[1]):
                self.ref.step(autoreset=op[0] == "steps", count=False)
        elif op[0] == "wd":
            v.weight[:] = wt
            v.degree[:] = dg
        return None

    def clash(self, e, ep):
        """make_game(env e, episode ep) redraws a start: its first two positions fall on one cell."""
        words = np.concatenate([self.oracle.philox([e, ep, 2, b], [self.ref.seed, self.ref.rank]) for b in range(12)])
        return self.oracle.make_game(self.W, self.fair, words)[3] > (9 if self.fair else 7)

    def counts(self, envs=0):
        """What the launches of the sequence handed over and took, from the oracle alone."""
        out = dict(launches=len(self.launches), handed=0, handed_behind_tape=0, full_last_block=0, idle_last_block=0,
                   step0=0, handed_clashes=0)
        for handed, tape, before, hit in self.launches:
            k = len(hit)
            lastb = hit[(k - 1) // R * R:]                           # the launch's last block
            out["full_last_block"] += int(lastb.all(0).sum())
            out["idle_last_block"] += int((~lastb.any(0)).sum())
            if handed:
                out["handed"] += 1
                out["step0"] += int(hit[0].sum())
                for e in range(min(envs, self.N)):                   # the ordinals (0, ROLL_R] this launch was handed
                    out["handed_clashes"] += sum(self.clash(e, int(before[e]) + j) for j in range(1, R + 1))
        prev_tape = [False] + [l[1] for l in self.launches[:-1]]
        out["handed_behind_tape"] = sum(1 for l, p in zip(self.launches, prev_tape) if l[0] and p and not l[1])
        return out


def model_sequence(oracle, N, W, fair, ops):
    """The ops on the oracle alone."""
    mod = Model(oracle, N, W, fair)
    rs = np.random.RandomState(1)
    for i, op in enumerate(ops):
        tape = None
        if op[0] in ("tape", "rec"):                                 # (any tape: no GPU here, the values need not be make_tape's)
            tape = rs.randint(0, 4, (op[1], N, 2)).astype(np.int8)
        mod.op(op, i, tape)
    return mod


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


@pytest.fixture(scope="module")
def twin(T, tmp_path_factory):
    """Every case of this file in one child process under TRON_ROLL_NO_HANDOFF: {case: {op tag: {field: digest}}}."""
    path = str(tmp_path_factory.mktemp("handoff") / "twin.json")
    env = dict(os.environ, TRON_ROLL_NO_HANDOFF="1")
    subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, timeout=600)
    with open(path) as f:
        return json.load(f)


def run_case(T, twin, name):
    tv, oracle = T
    N, W, fair, ops = CASES[name]
    mod = Model(oracle, N, W, fair)
    want = twin[name]
    seen = {}

    def after_op(i, op, got, rec, tape):
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
        rows = None
        if op is not None:
            rows = mod.op(op, i, None if tape is None else tape.cpu().numpy())
        check_against_oracle(got, ref, tag)
        if rec is not None:
            for field, g_, w_ in zip(("done", "winner", "reward"), rec, rows):
                w_ = w_.astype(g_.dtype)
                assert g_.shape == w_.shape and np.array_equal(g_.view(np.uint8), w_.view(np.uint8)), (tag, field, "oracle")
        assert digests(got, rec) == want.get(str(i)), (tag, "twin")
        return False

    gpu_sequence(tv, N, W, fair, ops, after_op)
    return mod.counts()


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("N", SMALL)
@pytest.mark.parametrize("W", SIDES)
def test_consecutive_rollouts(T, twin, W, N, fair):
    c = run_case(T, twin, f"rolls-{W}-{N}-{int(fair)}")
    assert c["launches"] == 12 and c["handed"] == 11                # 7 draws; 8 .. 64, two of 65 and three of 130 are handed


@pytest.mark.parametrize("N", (63, 257))
@pytest.mark.parametrize("W", SIDES)
@pytest.mark.parametrize("seq", ("mixed_a", "mixed_b"))
def test_instantiations_interleaved(T, twin, seq, W, N):
    c = run_case(T, twin, f"{seq}-{W}-{N}")
    assert c["launches"] == 12 and c["handed"] == 11 and c["handed_behind_tape"] >= 2


@pytest.mark.parametrize("N", (63, 257))
@pytest.mark.parametrize("W", SIDES)
def test_every_invalidating_call(T, twin, W, N):
    c = run_case(T, twin, f"invalidate-{W}-{N}")
    assert c["launches"] == 10 and c["handed"] == 6                 # the second rollout behind each call, both behind the refused attach


@pytest.mark.parametrize("N", (63, 257))
@pytest.mark.parametrize("W", SIDES)
def test_finished_on_entry(T, twin, W, N):
    c = run_case(T, twin, f"finished-{W}-{N}")
    assert c["launches"] == 4 and c["handed"] == 3


def test_four_game_waves_per_workgroup(T, twin):
    c = run_case(T, twin, "large-24")
    assert c["launches"] == 5 and c["handed"] == 4


def reached(oracle):
    """The counts test_inputs_reach_the_cases asserts on: the oracle alone, no GPU result enters."""
    out = {}
    c = model_sequence(oracle, 257, 4, False, ROLLS).counts(envs=16)
    out["env-launches that restart in every step of the last block (side 4, 257 envs, ROLLS)"] = c["full_last_block"]
    out["env-launches that restart in no step of the last block (side 4, 257 envs, ROLLS)"] = c["idle_last_block"]
    out["handed ordinals whose starts clash (side 4, first 16 envs, ROLLS)"] = c["handed_clashes"]
    out["env-launches whose step 0 restarts on a handed ordinal (side 4, 257 envs, ROLLS)"] = c["step0"]
    c = model_sequence(oracle, 257, 24, False, ROLLS).counts()
    out["env-launches that restart in every step of the last block (side 24, 257 envs, ROLLS)"] = c["full_last_block"]
    out["env-launches whose step 0 restarts on a handed ordinal (side 24, 257 envs, ROLLS)"] = c["step0"]
    c = model_sequence(oracle, 257, 10, False, MIXED_B).counts()
    out["launches that draw their actions behind a tape launch's hand-off (side 10, 257 envs, MIXED_B)"] = c["handed_behind_tape"]
    return out


def test_inputs_reach_the_cases(T):
    """Conditions on the oracle alone: the sequences above reach what they are there to reach."""
    out = reached(T[1])
    for k, v in out.items():
        print(f"{k}: {v}")
    for k, v in out.items():
        assert v > 0, k


def twin_main(path):
    """The child process: every case without an oracle, the digests of what each op left."""
    import torch
    import tron.vec as tv
    assert torch.cuda.is_available() and os.environ.get("TRON_ROLL_NO_HANDOFF")
    out = {}
    for name, (N, W, fair, ops) in CASES.items():
        seq = out[name] = {}
        ep = {}

        def after_op(i, op, got, rec, tape):
            if got is None:                                          # the tail: while some env has not restarted, by its own counters
                ep.setdefault("first", ep["now"])
                return not (ep["now"] != ep["first"]).all() and int(i.split("-")[1]) < FOLLOW_MAX
            ep["now"] = got["counters"][:, 1].copy()
            seq[str(i)] = digests(got, rec)
            return False

        gpu_sequence(tv, N, W, fair, ops, after_op)
    with open(path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    twin_main(sys.argv[1])
