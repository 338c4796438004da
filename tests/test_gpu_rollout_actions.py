"""tron_rollout_actions / VecTron.rollout_actions: K steps with autoreset whose actions come from the caller's tape.  What
the call leaves behind must be, bit for bit, what K calls of step(tape[k], autoreset=True) leave on a twin VecTron with
the same seed and the same reset(), and what the CPU oracle holds after the same tape: both observation planes, the board,
every field VecTron.state() shows and the totals.  All comparisons are exact and cover every env.

Shapes.  Mode None on the attached int8 codes runs k_obs_roll_tape: one lane per env, 64 envs per game wave, a helper wave
that copies the tape into the action ring one block of R = 8 steps ahead, launches of at most 64 steps.  A batch of no more
64-env waves than the chip has CUs gets ONE game wave per workgroup, so N = 1 is one lane of one wave, N = 70 a full
workgroup and a ragged second one, N = 200 four workgroups (the last one 8 lanes); the other split of the launch, FOUR game
waves (256 envs) per workgroup, needs more waves than CUs and is taken at N = 16 384 + 200 (65 workgroups, the last one a
ragged wave).  K = 1 (a single per-step launch), 63 / 64 / 65 (a short last block; exactly one launch; a second launch of
one step, its tape pointer advanced), 130 (three launches, the helper's ring wrapping eight times in each full one).  At
W = 4 a game fills its 16 cells in at most 7 steps, so every env restarts more often per launch than the restart ring's 16
slots (34 to 49 times in 64 steps under these tapes; 21 to 34 times at W = 10, whose longer trails cross launch boundaries).

The twin is stepped once per (mode, W, N) through the longest tape and its state kept at every K of interest: a tape of K
steps is the first K rows of that one.  Tapes are uniform over 0..3 from a seeded torch.Generator.
"""
import pytest

from rollout_support import Ref, check_against_oracle, check_against_twin, gpu_modules, make_tape, new_totals, pull, step_counted

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, RANK = 0x7A9E, 1
STATE_KEYS = ("pos", "alive", "dir", "done", "winner", "weight", "degree", "slide", "counters")
KS = (1, 63, 64, 65, 130)
FOUR_WAVES = 16384 + 200                                         # more 64-env waves than an MI355X has CUs (256)


@pytest.fixture(scope="module")
def tv():
    return gpu_modules()[0]


def make(tv, N, W, mode=None, obs_format="codes"):
    env = tv.VecTron(N, W, mode=mode, seed=SEED, rank=RANK, obs_format=obs_format)
    env.reset()
    return env, new_totals()


def assert_same(got, want, tag):
    assert set(want) == {"obs", "grid", "totals"} | set(STATE_KEYS)
    check_against_twin(got, want, tag)


_TWINS = {}


def twin_states(tv, mode, W, N, K):
    """The twin stepped through the (N, 130) tape, one launch per step, its state kept after every k of KS; returns the one
    after K steps.  Computed once per (mode, W, N) and never changed."""
    key = (mode, W, N)
    if key not in _TWINS:
        tape = make_tape(N, max(KS))
        twin, ttot = make(tv, N, W, mode)
        snaps = {}
        for k in range(max(KS)):
            step_counted(twin, ttot, tape[k])
            if k + 1 in KS:
                snaps[k + 1] = pull(twin, ttot)
        twin.close()
        _TWINS[key] = snaps
    return _TWINS[key][K]


def run_tape(tv, N, W, K, mode=None, **kw):
    env, totals = make(tv, N, W, mode)
    env.rollout_actions(make_tape(N, max(KS))[:K].contiguous(), totals, **kw)
    got = pull(env, totals)
    env.close()
    return got


# ---- 1: the tape rollout equals per-step stepping
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [1, 70, 200])
@pytest.mark.parametrize("W", [4, 10])
def test_tape_equals_per_step(tv, W, N, K):
    assert_same(run_tape(tv, N, W, K), twin_states(tv, None, W, N, K), (W, N, K))


@pytest.mark.parametrize("W,K", [(4, 130), (10, 65)])
def test_tape_equals_per_step_four_game_waves(tv, W, K):
    """256 envs and four helpers per workgroup (see the docstring): 200 does not reach that split, this batch does."""
    assert_same(run_tape(tv, FOUR_WAVES, W, K), twin_states(tv, None, W, FOUR_WAVES, K), (W, K))


def test_restarts_outnumber_the_restart_ring(tv):
    """(the per-step twin alone) at W = 4 every env restarts more than 16 times in a launch of 64 steps."""
    ep = twin_states(tv, None, 4, 70, 64)["counters"][:, 1]
    assert int(ep.min()) > 16


# ---- 2: the tape rollout equals the C oracle
def test_tape_equals_oracle(tv):
    import oracle
    N, W, K = 70, 10, 130
    tape = make_tape(N, max(KS))[:K].contiguous()
    ref = Ref(oracle, N, W, SEED, RANK)
    host = tape.cpu().numpy()
    for k in range(K):
        ref.step(host[k])
    env, totals = make(tv, N, W)
    env.rollout_actions(tape, totals)
    got = pull(env, totals)
    env.close()
    check_against_oracle(got, ref, "the oracle")
    assert int(ref.v.episode.min()) > 0                          # (the oracle alone) every env restarted under this tape


# ---- 3: a tape split over two calls
def test_split_tape(tv):
    N, W = 70, 4
    tape = make_tape(N, max(KS))
    env, totals = make(tv, N, W)
    env.rollout_actions(tape[:50].contiguous(), totals)
    env.rollout_actions(tape[50:130].contiguous(), totals)
    got = pull(env, totals)
    env.close()
    assert_same(got, twin_states(tv, None, W, N, 130), "50 + 80")


# ---- 4: tape launches and random launches on one handle
def test_interleaved_with_rollout_random(tv):
    N, W = 70, 10
    a, b = make_tape(N, 65, salt=1), make_tape(N, 3, salt=2)
    env, totals = make(tv, N, W)
    env.rollout_actions(a, totals)
    env.rollout_random(20, totals)
    env.rollout_actions(b, totals)
    twin, ttot = make(tv, N, W)
    for k in range(65):
        step_counted(twin, ttot, a[k])
    twin.rollout_random(20, ttot, per_step_launches=True)
    for k in range(3):
        step_counted(twin, ttot, b[k])
    assert_same(pull(env, totals), pull(twin, ttot), "65 tape, 20 random, 3 tape")
    env.close()
    twin.close()


# ---- 5: the paths that loop over the per-step launch
def test_fallback_temper(tv):
    assert_same(run_tape(tv, 70, 10, 20, mode="temper"), twin_by_steps(tv, 70, 10, 20, mode="temper"), "temper")


def test_fallback_odd_side(tv):
    assert_same(run_tape(tv, 70, 5, 20), twin_by_steps(tv, 70, 5, 20), "W = 5")


def twin_by_steps(tv, N, W, K, mode=None):
    tape = make_tape(N, max(KS))
    twin, ttot = make(tv, N, W, mode)
    for k in range(K):
        step_counted(twin, ttot, tape[k])
    got = pull(twin, ttot)
    twin.close()
    return got


def test_per_step_launches_flag(tv):
    assert_same(run_tape(tv, 70, 10, 65, per_step_launches=True), twin_states(tv, None, 10, 70, 65), "per_step_launches")


def test_fallback_f32_planes_on_attached_codes(tv):
    """The raw call with TRON_OBS_PLANES3_F32 on a handle whose codes are attached: per-step launches, then the planes."""
    nat = tv.nat
    N, W, K = 70, 10, 65
    env, totals = make(tv, N, W)
    tape = make_tape(N, max(KS))[:K].contiguous()
    planes = torch.empty(N, 2, 3, W + 2, W + 2, dtype=torch.float32, device="cuda")
    rc = env._lib.tron_rollout_actions(env._h, K, nat.ptr(tape), 0, nat.OBS_PLANES3_F32, nat.ptr(planes), nat.ptr(totals),
                                       nat.stream_ptr())
    assert rc == nat.OK
    want_planes = env.encode("planes3")
    got = pull(env, totals)
    assert torch.equal(planes, want_planes)
    env.close()
    assert_same(got, twin_states(tv, None, W, N, K), "f32 planes")


def test_bytes_outside_0_3_are_read_as_the_per_step_kernel_reads_them(tv):
    """The caller's error, but a defined one: both paths take the byte's low two bits."""
    N, W, K = 70, 10, 20
    tape = make_tape(N, K, salt=3, lo=-128, hi=128)
    assert int(tape.min()) < 0 and int(tape.max()) > 3
    env, totals = make(tv, N, W)
    env.rollout_actions(tape, totals)
    twin, ttot = make(tv, N, W)
    for k in range(K):
        step_counted(twin, ttot, tape[k])
    masked, mtot = make(tv, N, W)
    masked.rollout_actions(tape & 3, mtot)
    got = pull(env, totals)
    assert_same(got, pull(twin, ttot), "raw bytes")
    assert_same(got, pull(masked, mtot), "bytes & 3")
    for e in (env, twin, masked):
        e.close()


# ---- 6: arguments
def test_arguments(tv):
    nat = tv.nat
    N, W = 70, 10
    env, totals = make(tv, N, W)
    tape = make_tape(N, 4)
    before = pull(env, totals)

    def raw(k, actions, flags):
        return env._lib.tron_rollout_actions(env._h, k, nat.ptr(actions), flags, nat.OBS_CODES_I8, nat.ptr(env.obs),
                                             nat.ptr(totals), nat.stream_ptr())

    assert raw(4, None, 0) == nat.ERR_BAD_ARG
    assert raw(-1, tape, 0) == nat.ERR_BAD_ARG
    assert raw(4, tape, 64) == nat.ERR_BAD_ARG                   # an unknown bit
    for known_elsewhere in (nat.STEP_AUTORESET, nat.STEP_NONREVERSING, nat.ROLLOUT_TWO_STREAMS, nat.ROLLOUT_RESIDENT):
        assert raw(4, tape, known_elsewhere) == nat.ERR_BAD_ARG
    assert raw(0, tape, 0) == nat.OK
    assert_same(pull(env, totals), before, "nothing ran")

    with pytest.raises(ValueError):
        env.rollout_actions(make_tape(N + 1, 4))                 # shape
    with pytest.raises(ValueError):
        env.rollout_actions(tape[:, :, 0])
    with pytest.raises(TypeError):
        env.rollout_actions(tape.to(torch.int32))                # dtype
    with pytest.raises(ValueError):
        env.rollout_actions(tape.cpu())                          # a host tensor
    with pytest.raises(ValueError):
        env.rollout_actions(tape.transpose(0, 1).contiguous().transpose(0, 1))   # right shape, not contiguous
    with pytest.raises(TypeError):
        env.rollout_actions(tape.cpu().numpy())
    assert_same(pull(env, totals), before, "nothing ran")
    env.close()
