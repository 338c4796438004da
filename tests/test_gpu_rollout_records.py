"""tron_rollout_actions_records / VecTron.rollout_actions(records=...): the tape rollout that also records every step.  Row k
of the three record tapes (reward f32 [K, N, 2], done int8 [K, N], winner int8 [K, N]) must be, bit for bit, what the k-th
step(tape[k], autoreset=True) returns as (reward, done, winner) on a twin VecTron with the same seed and the same reset(),
and what the C oracle returns for the same tape; everything else the call leaves behind (both observation planes, the board,
every field VecTron.state() shows, the totals) must be what rollout_actions leaves, which is what the twin holds.  All
comparisons are exact and cover every env and every step.

Shapes (those of test_gpu_rollout_actions.py, for the same reasons).  Mode None on the attached int8 codes runs
k_obs_roll_tape_rec: one lane per env, 64 envs per game wave, launches of at most 64 steps, each launch's record rows behind
those of the launch before.  N = 1 is one lane of one wave, N = 70 a full workgroup and a ragged second one (6 lanes), N = 200
four workgroups (the last one 8 lanes); FOUR game waves per workgroup need more 64-env waves than the chip has CUs:
N = 16 384 + 200.  K = 1 (a single per-step launch), 63 / 64 / 65 (a short last block; exactly one launch; a second launch of
one step, whose record pointers are advanced), 130 (three launches).  At W = 4 a game ends within 7 steps, so every env
finishes many times per launch and the three winners all occur.  Two reward tables: the default one (a constant step reward)
and DQN's, whose step reward is the episode's step index (the eplen path of step_rewards).

The twin is stepped once per (reward table, mode, W, N) through the longest tape, its records stacked per step and its state
kept at every K of interest: a tape of K steps is the first K rows of that one.  Tapes are uniform over 0..3 from a seeded
torch.Generator.
"""
import ctypes as C

import numpy as np
import pytest

from rollout_support import check_against_twin, gpu_modules, make_tape, new_totals, pull, step_counted

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, RANK = 0x7A9E, 1
STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree", "slide", "counters")
KS = (1, 20, 63, 64, 65, 130)                                     # (20: the fallback tests' length)
FOUR_WAVES = 16384 + 200                                         # more 64-env waves than an MI355X has CUs (256)
REWARDS = {"default": None, "dqn": dict(step=0.0, win=100.0, lose=-25.0, draw=0.0, step_is_index=1)}
SENTINEL = 0x55
PRE_STEPS = 2                                                    # a 4x4 game lasts at most 7 steps: two end most and not all


@pytest.fixture(scope="module")
def tv():
    return gpu_modules()[0]


def make(tv, N, W, mode=None, reward="default"):
    env = tv.VecTron(N, W, mode=mode, seed=SEED, rank=RANK, obs_format="codes")
    if REWARDS[reward] is not None:
        env.set_reward(**REWARDS[reward])
    env.reset()
    return env, new_totals()


def assert_same(got, want, tag):
    assert set(want) == {"obs", "grid", "totals"} | set(STATE_KEYS)
    check_against_twin(got, want, tag)


def assert_records(got, want, K, tag, which=(0, 1, 2)):
    """got: (reward, done, winner) of a K-step call (device tensors or None); want: the twin's stacked records."""
    for i in which:
        g = got[i].cpu()
        assert g.dtype == want[i].dtype and g.shape == want[i][:K].shape, (tag, i)
        assert torch.equal(g.view(torch.uint8), want[i][:K].contiguous().view(torch.uint8)), (tag, ("reward", "done", "winner")[i])


def stack(rows):
    return tuple(torch.stack([r[i] for r in rows]).cpu() for i in range(3))


_TWINS = {}


def twin(tv, W, N, mode=None, reward="default"):
    """The twin stepped through the (N, 130) tape, one launch per step: (its state after every k of KS, its stacked records
    [130, ...] on the host).  Computed once per key and never changed."""
    key = (reward, mode, W, N)
    if key not in _TWINS:
        tape = make_tape(N, max(KS))
        env, tot = make(tv, N, W, mode, reward)
        snaps, rows = {}, []
        for k in range(max(KS)):
            rows.append(step_counted(env, tot, tape[k]))
            if k + 1 in KS:
                snaps[k + 1] = pull(env, tot)
        env.close()
        _TWINS[key] = (snaps, stack(rows))
    return _TWINS[key]


def run_records(tv, N, W, K, mode=None, reward="default", records=True, **kw):
    env, totals = make(tv, N, W, mode, reward)
    rec = env.rollout_actions(make_tape(N, max(KS))[:K].contiguous(), totals, records=records, **kw)
    got = pull(env, totals)
    env.close()
    return rec, got


def check_records_against_twin(tv, N, W, K, tag, mode=None, reward="default", **kw):
    rec, got = run_records(tv, N, W, K, mode, reward, **kw)
    snaps, want = twin(tv, W, N, mode, reward)
    assert rec[0].shape == (K, N, 2) and rec[1].shape == (K, N) and rec[2].shape == (K, N)
    assert_records(rec, want, K, tag)
    assert_same(got, snaps[K], tag)


# ---- 1: the records equal the per-step twin's
@pytest.mark.parametrize("reward", ["default", "dqn"])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("N", [1, 70, 200])
@pytest.mark.parametrize("W", [4, 10])
def test_records_equal_per_step(tv, W, N, K, reward):
    check_records_against_twin(tv, N, W, K, (W, N, K, reward), reward=reward)


def test_the_twin_pays_by_step_index_under_the_dqn_table(tv):
    """(the twin alone) the second table makes the eplen path live: its records differ from the default table's."""
    a, b = twin(tv, 4, 70)[1], twin(tv, 4, 70, reward="dqn")[1]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and not torch.equal(a[0], b[0])


# ---- 2: four game waves per workgroup
def test_records_four_game_waves(tv):
    check_records_against_twin(tv, FOUR_WAVES, 4, 130, "four game waves")


# ---- 3: the C oracle
def test_records_equal_oracle(tv):
    import oracle
    N, W, K = 70, 10, 130
    tape = make_tape(N, max(KS))[:K].contiguous()
    ref = oracle.VecOracle(N, W, seed=SEED, stream=RANK)
    ref.reset_all()
    host = tape.cpu().numpy()
    rows = [ref.step(actions=host[k], autoreset=True, want_obs=False)[1:] for k in range(K)]
    d, w, r = (np.stack([np.array(row[i]) for row in rows]) for i in range(3))
    for winner in (0, 1, 2):                                     # (the oracle alone) the tape finishes games every way
        assert int(((d == 1) & (w == winner)).sum()) > 0, winner
    env, totals = make(tv, N, W)
    reward, done, winner = env.rollout_actions(tape, totals, records=True)
    torch.cuda.synchronize()
    assert np.array_equal(done.cpu().numpy(), d.astype(np.int8))
    assert np.array_equal(winner.cpu().numpy(), w.astype(np.int8))
    assert r.dtype == np.float32 and np.array_equal(reward.cpu().numpy().view(np.uint32), r.view(np.uint32))
    assert np.array_equal(env.grid().cpu().numpy().reshape(N, -1), ref.grid)
    env.close()


# ---- 4: envs that are finished when the tape begins
def test_envs_finished_on_entry(tv):
    N, W, K = 70, 4, 65
    pre, tape = make_tape(N, 8, salt=5), make_tape(N, K, salt=6)
    a, atot = make(tv, N, W)
    b, btot = make(tv, N, W)
    for k in range(PRE_STEPS):
        a.step(pre[k], autoreset=False)
        b.step(pre[k], autoreset=False)
    fin = b.state()["done"]
    assert int((fin == 1).sum()) > 0 and int((fin == 0).sum()) > 0
    rec = a.rollout_actions(tape, atot, records=True)
    want = stack([step_counted(b, btot, tape[k], live=(fin == 0) if k == 0 else None) for k in range(K)])
    assert_records(rec, want, K, "finished on entry")
    assert bool((want[1][0][fin.cpu() == 1] == 1).all())         # such an env's first row says done: it restarts without a move
    assert_same(pull(a, atot), pull(b, btot), "finished on entry")
    a.close()
    b.close()


# ---- 5: any subset of the three tapes
@pytest.mark.parametrize("which", [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), ()])
def test_subsets(tv, which):
    N, W, K = 70, 4, 130
    env, totals = make(tv, N, W, reward="dqn")
    shapes = ((K, N, 2), (K, N), (K, N))
    dtypes = (torch.float32, torch.int8, torch.int8)
    asked = tuple(torch.empty(shapes[i], dtype=dtypes[i], device="cuda") if i in which else None for i in range(3))
    back = env.rollout_actions(make_tape(N, max(KS))[:K].contiguous(), totals, records=asked)
    assert back is asked
    snaps, want = twin(tv, W, N, reward="dqn")
    assert_records(asked, want, K, which, which)
    assert_same(pull(env, totals), snaps[K], which)
    env.close()


# ---- 6: nothing outside the rows
@pytest.mark.parametrize("N", [70, 200])
def test_nothing_outside_the_rows(tv, N):
    W, K = 4, 65
    env, totals = make(tv, N, W)
    reward = torch.empty(K + 2, N, 2, dtype=torch.float32, device="cuda")
    done = torch.empty(K + 2, N, dtype=torch.int8, device="cuda")
    winner = torch.empty(K + 2, N, dtype=torch.int8, device="cuda")
    for t in (reward, done, winner):
        t.view(torch.uint8).fill_(SENTINEL)
    views = (reward[1:K + 1], done[1:K + 1], winner[1:K + 1])
    assert all(v.is_contiguous() for v in views)
    env.rollout_actions(make_tape(N, max(KS))[:K].contiguous(), totals, records=views)
    torch.cuda.synchronize()
    for t in (reward, done, winner):
        guard = t.view(torch.uint8).cpu()
        assert bool((guard[0] == SENTINEL).all()) and bool((guard[K + 1] == SENTINEL).all())
    snaps, want = twin(tv, W, N)
    assert_records(views, want, K, ("guard rows", N))
    assert_same(pull(env, totals), snaps[K], ("guard rows", N))
    env.close()


# ---- 7: a tape split over two calls, into views of one record buffer
def test_split_tape(tv):
    N, W, K = 70, 4, 130
    tape = make_tape(N, max(KS))
    env, totals = make(tv, N, W)
    reward = torch.empty(K, N, 2, dtype=torch.float32, device="cuda")
    done = torch.empty(K, N, dtype=torch.int8, device="cuda")
    winner = torch.empty(K, N, dtype=torch.int8, device="cuda")
    env.rollout_actions(tape[:50].contiguous(), totals, records=(reward[:50], done[:50], winner[:50]))
    env.rollout_actions(tape[50:130].contiguous(), totals, records=(reward[50:], done[50:], winner[50:]))
    snaps, want = twin(tv, W, N)
    assert_records((reward, done, winner), want, K, "50 + 80")
    assert_same(pull(env, totals), snaps[K], "50 + 80")
    env.close()


# ---- 8: the paths that loop over the per-step launch
def test_fallback_temper(tv):
    check_records_against_twin(tv, 70, 10, 20, "temper", mode="temper")


def test_fallback_odd_side(tv):
    check_records_against_twin(tv, 70, 5, 20, "W = 5")


def test_per_step_launches_flag(tv):
    check_records_against_twin(tv, 70, 10, 65, "per_step_launches", per_step_launches=True)


def test_fallback_f32_planes_on_attached_codes(tv):
    """The raw call with TRON_OBS_PLANES3_F32 on a handle whose codes are attached: per-step launches, then the planes."""
    nat = tv.nat
    N, W, K = 70, 10, 65
    env, totals = make(tv, N, W)
    tape = make_tape(N, max(KS))[:K].contiguous()
    planes = torch.empty(N, 2, 3, W + 2, W + 2, dtype=torch.float32, device="cuda")
    rec = (torch.empty(K, N, 2, dtype=torch.float32, device="cuda"), torch.empty(K, N, dtype=torch.int8, device="cuda"),
           torch.empty(K, N, dtype=torch.int8, device="cuda"))
    rc = env._lib.tron_rollout_actions_records(env._h, K, nat.ptr(tape), 0, nat.OBS_PLANES3_F32, nat.ptr(planes), nat.ptr(rec[1]),
                                               nat.ptr(rec[2]), nat.ptr(rec[0]), nat.ptr(totals), nat.stream_ptr())
    assert rc == nat.OK
    assert torch.equal(planes, env.encode("planes3"))
    snaps, want = twin(tv, W, N)
    assert_records(rec, want, K, "f32 planes")
    assert_same(pull(env, totals), snaps[K], "f32 planes")
    env.close()


# ---- 9: arguments
def test_arguments(tv):
    nat = tv.nat
    N, W, K = 70, 10, 4
    env, totals = make(tv, N, W)
    tape = make_tape(N, K)
    reward = torch.empty(K + 1, N, 2, dtype=torch.float32, device="cuda")
    done = torch.empty(K, N, dtype=torch.int8, device="cuda")
    winner = torch.empty(K, N, dtype=torch.int8, device="cuda")
    bufs = (reward, done, winner)
    for t in bufs:
        t.view(torch.uint8).fill_(SENTINEL)
    before = pull(env, totals)

    def raw(k, actions, flags, reward_ptr=nat.ptr(reward)):
        return env._lib.tron_rollout_actions_records(env._h, k, nat.ptr(actions), flags, nat.OBS_CODES_I8, nat.ptr(env.obs),
                                                     nat.ptr(done), nat.ptr(winner), reward_ptr, nat.ptr(totals), nat.stream_ptr())

    def untouched(tag):
        assert_same(pull(env, totals), before, tag)
        for t in bufs:
            assert bool((t.view(torch.uint8) == SENTINEL).all()), tag

    assert raw(K, None, 0) == nat.ERR_BAD_ARG
    assert raw(-1, tape, 0) == nat.ERR_BAD_ARG
    assert raw(K, tape, 64) == nat.ERR_BAD_ARG                   # an unknown bit
    assert raw(K, tape, 0, C.c_void_p(reward.data_ptr() + 4)) == nat.ERR_BAD_ARG    # float2 rows: 8-byte aligned
    untouched("bad arguments")
    assert raw(0, tape, 0) == nat.OK
    untouched("k_steps == 0")

    none = env.rollout_actions(tape[:0], totals, records=True)   # K == 0: empty tensors, nothing launched
    assert tuple(none[0].shape) == (0, N, 2) and tuple(none[1].shape) == (0, N) and tuple(none[2].shape) == (0, N)
    assert none[0].dtype == torch.float32 and none[1].dtype == torch.int8 and none[2].dtype == torch.int8
    assert env.rollout_actions(tape[:0], totals) is None
    untouched("K == 0")

    ok = (reward[:K], done, winner)

    def swap(i, t):
        return tuple(t if j == i else ok[j] for j in range(3))

    for i in range(3):
        with pytest.raises(TypeError):
            env.rollout_actions(tape, totals, records=swap(i, ok[i].to(torch.float64)))          # dtype
        with pytest.raises(ValueError):
            env.rollout_actions(tape, totals, records=swap(i, ok[i][:K - 1]))                    # rows
        with pytest.raises(ValueError):
            env.rollout_actions(tape, totals, records=swap(i, ok[i].cpu()))                      # a host tensor
        with pytest.raises(ValueError):
            env.rollout_actions(tape, totals, records=swap(i, ok[i].transpose(0, 1).contiguous().transpose(0, 1)))
        with pytest.raises(TypeError):
            env.rollout_actions(tape, totals, records=swap(i, ok[i].cpu().numpy()))
    with pytest.raises(ValueError):
        env.rollout_actions(tape, totals, records=(reward[:K, :, 0], done, winner))              # [K, N] is no reward tape
    with pytest.raises(TypeError):
        env.rollout_actions(tape, totals, records=(reward[:K], done))
    untouched("rejected records")
    env.close()
