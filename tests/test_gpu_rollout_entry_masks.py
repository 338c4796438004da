"""k_obs_roll's masked entry.  Every launch of the roll_resident family (tron_rollout_random, tron_rollout_actions,
tron_rollout_actions_records on the attached int8 codes, mode None) leaves one 64-bit mask per env: the 16-cell chunks of the
player-1 plane that may differ from the fresh board.  The next such launch, if no other call that can write the planes or the
state words was enqueued in between, reads only those chunks instead of every env's whole plane; everything else is entered as
"the template".  The host keeps one flag per handle for "the masks describe the planes", cleared by every other entry point.

What a call leaves behind must be, bit for bit, what the CPU oracle holds after the same steps and what a twin VecTron holds
that makes every step a launch of its own (per_step_launches=True, which also never enters masked): both observation planes,
the board, every field of VecTron.state() (pos, alive, dir, done, winner, weight, degree, counters), the totals and, where a
call records, the three record tapes.  rs4's next-game words show as pos / weight / degree after an env's next restart, so
every sequence ends with per-step launches until every env has restarted again.

Shapes.  Sides 4 (3 chunks, the last one short), 10, 24 (43 chunks, the last one short), 30 (64 chunks: bit 63); envs 1, 39,
64, 65, 257 (one game wave per workgroup, ragged) and 16 385 at side 24 / 16 584 at side 30 (four / three game waves per
workgroup, the last workgroup with waves that have no env); `fair` on and off; both action policies.
Sequences.  ROLLS: consecutive rollouts of 1, 7, 8, 9, 63, 64, 65 and 130 steps — the one-step call is a per-step launch, the
7-step call enters by the full read, every later launch enters masked, the second and third launch of the 130-step call
included.  INVALIDATE: between two rollouts each call that clears the flag, once: a full reset, a masked reset, steps without
autoreset (the next rollout enters with finished envs), a step with autoreset, a part step, an incremental step, attaching
another buffer and the same one again (both refused by the library: the buffer stays), set_weight_degree; behind each the
next rollout must read whole planes and the one after it enters masked again.  MIXED: rollout_random, rollout_actions and
rollout_actions(records=True) interleaved, so that a mask written by one instantiation is read by another.  LONG: the
non-reversing policy over launches of 64 steps, whose games last: entry masks of many chunks.

Under autoreset no env is finished when a launch ends, and a head lies on a border cell of the board only in a finished game.
The short last chunk of sides 4 and 24 and chunk 63 of side 30 are border cells only.  So "entered finished", "the short last
chunk in the mask" and "bit 63" occur at the entry that follows steps without autoreset — a full read, whose launch then
writes the masks the next one enters by — and never at a masked entry; they are counted there.

test_inputs_reach_the_cases asserts on the oracle alone that the inputs reach the cases they are there for.
"""
import numpy as np
import pytest

from rollout_support import LAUNCH, Ref, check_against_oracle, check_against_twin, gpu_modules, make_tape, new_totals, \
    pull, restore_threads

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, RANK = 0xE7A5, 3
SIDES = (4, 10, 24, 30)
SMALL = (1, 39, 64, 65, 257)
LARGE = {24: 16384 + 1, 30: 16584}                               # four game waves of 64 at side 24, three at side 30
WAVES = {24: 4, 30: 3}
FOLLOW_MAX = 64                                                  # per-step launches after a sequence, at the most
ROLLS = [("roll", k) for k in (1, 7, 8, 9, 63, 64, 65, 130)]
INVALIDATE = [("roll", 9), ("reset",), ("roll", 9), ("roll", 65), ("reset_mask",), ("roll", 9), ("roll", 9),
              ("steps_noreset", 5), ("roll", 17), ("roll", 9), ("steps", 2), ("roll", 9), ("roll", 9), ("part",), ("roll", 9),
              ("roll", 9), ("inc",), ("roll", 9), ("roll", 9), ("attach_other",), ("roll", 9), ("roll", 9), ("attach_same",),
              ("roll", 9), ("roll", 9), ("wd",), ("roll", 9), ("roll", 9)]
MIXED = [("roll", 9), ("tape", 9), ("rec", 65), ("roll", 8), ("rec", 7), ("tape", 130), ("roll", 65), ("tape", 2), ("rec", 130),
         ("roll", 9)]
FINISHED = [("roll", 9), ("steps_noreset", 5), ("roll", 65), ("roll", 9)]
LONG = [("roll", 64), ("roll", 130), ("roll", 64)]


@pytest.fixture(scope="module")
def T():
    tv, oracle = gpu_modules(threads=True)
    yield tv, oracle
    restore_threads(oracle)


def op_inputs(N, W, i):
    """The arguments of the i-th op of a sequence (a masked reset's mask, set_weight_degree's values)."""
    rs = np.random.RandomState(7919 * W + 31 * i + N)
    m = (rs.rand(N) < 0.4).astype(np.int8)
    m[0] = 1
    wt = rs.randint(40, 102, (N, 2)).astype(np.int16)
    dg = rs.randint(-30, 31, N).astype(np.int16)
    return m, wt, dg


class Model:
    """The oracle side of a sequence: a Ref, the host flag as the issue states it (`valid`: the last op was a persistent
    launch) and, per launch of the roll_resident family, a note of what it entered with."""

    def __init__(self, oracle, N, W, fair):
        self.ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
        self.N, self.W, self.G = N, W, (W + 2) * (W + 2)
        self.cpe = (self.G + 15) // 16
        self.fresh = np.where(self.ref.border, -1, 1).astype(np.int8)    # the fresh board's player-1 plane
        self.valid = False
        self.notes = []

    def note(self):
        ref = self.ref
        p1 = ref.oracle.state_for_player(ref.v.grid, 1).reshape(self.N, -1)
        diff = np.pad(p1 != self.fresh, ((0, 0), (0, 16 * self.cpe - self.G))).reshape(self.N, self.cpe, 16).any(2)
        h1, h2 = p1 == 10, p1 == -10
        both = h1.any(1) & h2.any(1)
        same = both & (h1.argmax(1) // 16 == h2.argmax(1) // 16)
        self.notes.append(dict(masked=self.valid, diff=diff, done=ref.v.done == 1, same=same))

    def launches(self, K, nonrev=False, tape=None):
        """K steps with autoreset as a rollout call makes them; the (done, winner, reward) rows of every step."""
        rows = []
        if K < 2:                                                    # a single step is a per-step launch
            self.valid = False
        for k0 in range(0, K, LAUNCH):
            if K >= 2:
                self.note()
            for s in range(k0, min(K, k0 + LAUNCH)):
                rows.append(self.ref.step(actions=None if tape is None else tape[s], nonrev=nonrev))
            self.valid = K >= 2
        return tuple(np.stack([r[i] for r in rows]) for i in range(3))


def make(tv, N, W, fair):
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes", fair=fair)
    assert env.obs_is_state
    env.reset()
    return env, new_totals()


def gpu_op(tv, env, totals, op, i, nonrev, per_step, tape):
    """One op on a VecTron; the record tapes of a ("rec", K) op on the host, else None."""
    N, W = env.N, env.W
    m, wt, dg = op_inputs(N, W, i)
    if op[0] == "roll":
        env.rollout_random(op[1], totals, nonreversing=nonrev, per_step_launches=per_step)
    elif op[0] == "tape":
        env.rollout_actions(tape, totals, per_step_launches=per_step)
    elif op[0] == "rec":
        reward, done, winner = env.rollout_actions(tape, totals, per_step_launches=per_step, records=True)
        torch.cuda.synchronize()
        return done.cpu().numpy(), winner.cpu().numpy(), reward.cpu().numpy()
    elif op[0] == "reset":
        env.reset()
    elif op[0] == "reset_mask":
        env.reset(mask=torch.from_numpy(m))
    elif op[0] in ("steps", "steps_noreset"):
        for _ in range(op[1]):
            env.step(autoreset=op[0] == "steps", nonreversing=nonrev)
    elif op[0] == "part":
        if per_step:
            env.step()
        else:
            for p in range(2):                                       # the two halves of one step
                env.step_part(p, 2)
    elif op[0] == "inc":
        env.incremental = not per_step                              # (the twin makes the same step by the full rewrite)
        env.step()
        env.incremental = False
    elif op[0] in ("attach_other", "attach_same"):
        buf = env.obs if op[0] == "attach_same" else torch.zeros_like(env.obs)
        with torch.cuda.device(env.device):
            rc = env._lib.tron_attach_obs_state(env._h, tv.nat.ptr(buf), tv.nat.stream_ptr())
        assert rc != 0                                               # already attached: refused, the buffer stays
    elif op[0] == "wd":
        env.set_weight_degree(torch.from_numpy(wt), torch.from_numpy(dg))
    else:
        raise ValueError(op)
    return None


def model_op(mod, op, i, nonrev, tape):
    v = mod.ref.v
    m, wt, dg = op_inputs(mod.N, mod.W, i)
    if op[0] in ("roll", "tape", "rec"):
        return mod.launches(op[1], nonrev if op[0] == "roll" else False, tape)
    mod.valid = False
    if op[0] == "reset":
        v.reset_all()
    elif op[0] == "reset_mask":
        v.reset_masked(m)
    elif op[0] in ("steps", "steps_noreset"):
        for _ in range(op[1]):
            mod.ref.step(nonrev=nonrev, autoreset=op[0] == "steps", count=False)
    elif op[0] in ("part", "inc"):
        mod.ref.step(count=False)
    elif op[0] == "wd":
        v.weight[:] = wt
        v.degree[:] = dg
    return None


def run_sequence(T, N, W, fair, nonrev, ops, gpu=True):
    """The ops on the oracle, on a VecTron and on its per-step twin, compared after every op; the Model.  gpu=False: the
    oracle alone."""
    tv, oracle = T
    mod = Model(oracle, N, W, fair)
    if gpu:
        env, totals = make(tv, N, W, fair)
        twin, ttot = make(tv, N, W, fair)
    for i, op in enumerate(ops):
        tag = (N, W, fair, nonrev, i, op)
        tape = make_tape(N, op[1], salt=i) if op[0] in ("tape", "rec") else None      # (the tape ops need a device)
        host = None if tape is None else tape.cpu().numpy()
        want = model_op(mod, op, i, nonrev, host)
        if not gpu:
            continue
        rec = gpu_op(tv, env, totals, op, i, nonrev, False, tape)
        trec = gpu_op(tv, twin, ttot, op, i, nonrev, True, tape)
        got = pull(env, totals)
        check_against_oracle(got, mod.ref, tag)
        check_against_twin(got, pull(twin, ttot), tag + ("twin",))
        if op[0] == "rec":
            for name, g_, t_, w_ in zip(("done", "winner", "reward"), rec, trec, want):
                assert g_.shape == t_.shape and np.array_equal(g_.view(np.uint8), t_.view(np.uint8)), (tag, name, "twin")
                w_ = w_.astype(g_.dtype)
                assert g_.shape == w_.shape and np.array_equal(g_.view(np.uint8), w_.view(np.uint8)), (tag, name, "oracle")
    if gpu:
        # rs4.nstart / rs4.nenvp of every env: per-step launches with uniform actions until every env has restarted again
        ref = mod.ref
        seen = ref.v.episode.copy()
        for j in range(FOLLOW_MAX):
            if (ref.v.episode != seen).all():
                break
            ref.step(count=False)
            env.step()
            twin.step()
            check_against_oracle(pull(env, totals), ref, (N, W, fair, nonrev, "follow", j))
        assert (ref.v.episode != seen).all()                     # (the oracle alone) the next game of every env was looked at
        check_against_twin(pull(env, totals), pull(twin, ttot), (N, W, fair, nonrev, "follow", "twin"))
        env.close()
        twin.close()
    return mod


def counts(mod):
    """What the launches of a sequence entered with, from the oracle alone."""
    tail = mod.G % 16 != 0
    out = dict(masked=0, chunks3=0, max_chunks=0, last_short=0, bit63=0, finished=0, same_chunk=0, trips2=0, empty_waves=0)
    for n in mod.notes:
        per_env = n["diff"].sum(1)
        out["finished"] += int(n["done"].sum())
        if tail:
            out["last_short"] += int(n["diff"][:, -1].sum())
        if mod.cpe == 64:
            out["bit63"] += int(n["diff"][:, 63].sum())
        if not n["masked"]:
            continue
        out["masked"] += 1
        out["chunks3"] += int((per_env >= 3).sum())
        out["max_chunks"] = max(out["max_chunks"], int(per_env.max()))
        out["same_chunk"] += int(n["same"].sum())
        out["trips2"] += sum(int(per_env[w0:w0 + 64].sum() > 64) for w0 in range(0, mod.N, 64))
        if mod.N > 16384:                                            # waves of the last workgroup that have no env
            E = 64 * WAVES[mod.W]
            left = mod.N % E
            out["empty_waves"] += 0 if left == 0 else WAVES[mod.W] - (left + 63) // 64
    return out


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N", SMALL)
@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("W", SIDES)
def test_consecutive_rollouts(T, W, fair, N, nonrev):
    c = counts(run_sequence(T, N, W, fair, nonrev, ROLLS))
    assert c["masked"] == 9                                          # 8, 9, 63, 64, two of 65 and three of 130


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("W", (24, 30))
def test_consecutive_rollouts_full_workgroups(T, W, nonrev):
    """More 64-env waves than the chip has CUs: four game waves per workgroup at side 24, three at side 30; the last
    workgroup has waves without an env."""
    c = counts(run_sequence(T, LARGE[W], W, False, nonrev, ROLLS[3:]))
    assert c["masked"] == 7 and c["empty_waves"] > 0 and c["trips2"] > 0


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("N", (65, 257))
@pytest.mark.parametrize("W,fair", [(4, False), (10, True), (24, False), (30, False)])
def test_every_invalidating_call(T, W, fair, N, nonrev):
    c = counts(run_sequence(T, N, W, fair, nonrev, INVALIDATE))
    assert c["masked"] == 10 and c["finished"] > 0                  # the second rollout behind each call, and roll 65's second launch


@pytest.mark.parametrize("N", (39, 257))
@pytest.mark.parametrize("W,fair", [(4, True), (10, False), (24, False), (30, False)])
def test_instantiations_interleaved(T, W, fair, N):
    c = counts(run_sequence(T, N, W, fair, False, MIXED))
    assert c["masked"] == 15                                         # every launch of the sixteen but the first


@pytest.mark.parametrize("W", (24, 30))
def test_finished_envs_full_workgroups(T, W):
    """Steps without autoreset at the large shapes: heads on the border's last chunk (the short one at side 24, bit 63 at
    side 30) enter the full-read launch whose masks the next launch reads."""
    c = counts(run_sequence(T, LARGE[W], W, False, False, FINISHED))
    assert c["finished"] > 0 and (c["last_short"] if W == 24 else c["bit63"]) > 0 and c["masked"] == 2


@pytest.mark.parametrize("N", (64, 257))
@pytest.mark.parametrize("W", (24, 30))
def test_masks_grow_under_the_nonreversing_policy(T, W, N):
    c = counts(run_sequence(T, N, W, False, True, LONG))
    assert c["masked"] == 4 and c["max_chunks"] >= 6


def reached(T):
    """The counts test_inputs_reach_the_cases asserts on: the oracle alone, no GPU result enters."""
    out = {}
    c = counts(run_sequence(T, 257, 24, False, False, ROLLS, gpu=False))
    out["env-launches entered masked with >= 3 chunks in the mask (side 24, 257 envs, ROLLS)"] = c["chunks3"]
    out["env-launches entered masked with both heads in one chunk (side 24, 257 envs, ROLLS)"] = c["same_chunk"]
    out["wave-launches entered masked whose list needs more than one trip (side 24, 257 envs, ROLLS)"] = c["trips2"]
    c = counts(run_sequence(T, 257, 4, False, False, INVALIDATE, gpu=False))
    out["env-launches entered with the short last chunk in the mask (side 4, 257 envs, INVALIDATE)"] = c["last_short"]
    out["env-launches entered finished (side 4, 257 envs, INVALIDATE)"] = c["finished"]
    c = counts(run_sequence(T, LARGE[24], 24, False, False, FINISHED, gpu=False))
    out["env-launches entered with the short last chunk in the mask (side 24, 16 385 envs, FINISHED)"] = c["last_short"]
    out["wave-launches entered masked with no env (side 24, 16 385 envs, FINISHED)"] = c["empty_waves"]
    c = counts(run_sequence(T, LARGE[30], 30, False, False, FINISHED, gpu=False))
    out["env-launches entered with bit 63 in the mask (side 30, 16 584 envs, FINISHED)"] = c["bit63"]
    out["env-launches entered finished (side 30, 16 584 envs, FINISHED)"] = c["finished"]
    out["wave-launches entered masked with no env (side 30, 16 584 envs, FINISHED)"] = c["empty_waves"]
    c = counts(run_sequence(T, 257, 24, False, True, LONG, gpu=False))
    out["the largest mask at a masked entry, in chunks, minus 5 (side 24, 257 envs, LONG)"] = c["max_chunks"] - 5
    return out


def test_inputs_reach_the_cases(T):
    """Conditions on the oracle alone: the sequences above reach what they are there to reach."""
    out = reached(T)
    for k, v in out.items():
        print(f"{k}: {v}")
    for k, v in out.items():
        assert v > 0, k
