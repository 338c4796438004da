"""k_obs_roll's straight-line restart draw and its lean store loop.  What they can get wrong: a start whose two players
clash leaves the straight-line draw for the general routine, and every later draw of that game (the weights, the degree)
moves down the stream with it; the short last chunk of a plane is stored by a branch of its own and must stop at G; the
player-2 plane is made from the packed board in nibble space, not from the player-1 bytes.

Every byte of env.obs, grid() and state() and the totals are compared with the CPU oracle driven the same way; no
tolerances (the helpers are those of test_gpu_rollout_wave.py, restated).  The next game's start, weights and degree are
drawn one restart ahead and are not in state(): they are compared when the restart after puts them there."""
import numpy as np
import pytest

from rollout_support import Ref, check_against_oracle, gpu_modules, new_totals, np_, pull

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DOWN = 2                       # Direction index of a move to the next row (player.py:124-132)
CODES = (1, -1, -2, -3, 10, -10)
RESET_BLOCKS = 12              # Philox blocks a start can use: 2 + 4 + 2 * 16 + 3 draws


@pytest.fixture(scope="module")
def T():
    return gpu_modules()


def redraws_of_start(oracle, W, fair, seed, rank, env, episode):
    """How many times util.make_game redrew player 1 for the game (env, episode): each redraw takes two more draws."""
    base = 9 if fair else 7
    s = np.zeros(4 * RESET_BLOCKS, np.uint32)
    for b in range(3):
        s[4 * b:4 * b + 4] = oracle.philox([env, episode, 2, b], [seed, rank])
    n = oracle.make_game(W, fair, s)[3]
    if n > base:                                    # a clash: the stream goes on
        for b in range(3, RESET_BLOCKS):
            s[4 * b:4 * b + 4] = oracle.philox([env, episode, 2, b], [seed, rank])
        n = oracle.make_game(W, fair, s)[3]
    assert (n - base) % 2 == 0
    return (n - base) // 2


def count_redraws(ref, fin):
    """Ref's look at the finished envs before they restart: counts the restarts whose start was redrawn."""
    for i in np.flatnonzero(fin):
        n = redraws_of_start(ref.oracle, ref.W, ref.fair, ref.seed, ref.rank, int(i), int(ref.v.episode[i]))
        ref.restarts += 1
        ref.redrew_once += n >= 1
        ref.redrew_twice += n >= 2


def check(env, ref, tag):
    """Every byte a caller can read back against the oracle."""
    check_against_oracle(pull(env), ref, tag, totals=False)


def rollout(env, ref, K, tag=""):
    """K steps both ways; the rollout's totals against the oracle's."""
    totals = new_totals()
    env.rollout_random(K, totals)
    before = ref.totals.copy()
    for _ in range(K):
        ref.step()
    check(env, ref, f"rollout of {K} {tag}")
    assert np.array_equal(np_(totals), ref.totals - before), f"totals of the rollout of {K} {tag}"


def make(T, N, W, seed, rank, fair=False, count=False):
    tv, oracle = T
    env = tv.VecTron(N, W, fair=fair, seed=seed, rank=rank, obs_format="codes")
    assert env.obs_is_state
    env.reset()
    ref = Ref(oracle, N, W, seed, rank, fair=fair, before_restart=count_redraws if count else None)
    ref.restarts = ref.redrew_once = ref.redrew_twice = 0
    return env, ref


# Seeds for W = 4, fair=False, checked on the CPU with the oracle alone (the 133 steps of the test, this file's Ref): restarts
# whose start was redrawn at least once / at least twice: N = 1: 3 / 1 of 79; 64: 334 / 23 of 5 401; 65: 355 / 19 of 5 460;
# 200: 1 034 / 66 of 16 842.  A start clashes once in W^2 = 16 times; one env alone needs a seed that shows a second redraw.
CLASH_SEED = {1: 1, 64: 164, 65: 165, 200: 300}


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("W", [4, 6])
@pytest.mark.parametrize("N", [1, 64, 65, 200])
def test_clash_redraws_through_the_rollout(T, N, W, fair):
    """Rollouts of 1, 3, 64 and 65 steps one after another on boards small enough that starts clash all the time: the
    lanes that clash leave the straight-line draw, singly and repeatedly, beside lanes that do not."""
    count = W == 4 and not fair
    env, ref = make(T, N, W, seed=CLASH_SEED[N], rank=2, fair=fair, count=count)
    check(env, ref, "reset")
    for K in (1, 3, 64, 65):
        rollout(env, ref, K, tag=f"N={N} W={W} fair={fair}")
    if count:
        print(f"restarts {ref.restarts}, redrawn at least once {ref.redrew_once}, at least twice {ref.redrew_twice}")
        assert ref.redrew_once > 0 and ref.redrew_twice > 0, "the seed must take the redraw path, once and repeatedly"


@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("W", [4, 10])
def test_make_game_in_every_caller(T, W, fair):
    """tron_reset (whole batch and masked: this game and the next), steps with the caller's actions and autoreset (the
    per-step kernels), incremental steps and rollouts, each through enough restarts that the starts, weights and degrees
    drawn one game ahead come up in state()."""
    N = 130
    env, ref = make(T, N, W, seed=91 + W, rank=3, fair=fair)
    rs = np.random.RandomState(W + int(fair))
    check(env, ref, "reset")
    for k in range(8):
        acts = rs.randint(0, 4, (N, 2)).astype(np.int8)
        _, reward, done, winner = env.step(torch.from_numpy(acts))
        d, w, r = ref.step(acts)
        assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
        check(env, ref, f"step {k} with the caller's actions")
    rollout(env, ref, 9, tag="after steps with actions")
    env.incremental = True
    for k in range(8):
        env.step()
        ref.step()
        check(env, ref, f"incremental step {k}")
    env.incremental = False
    rollout(env, ref, 9, tag="after incremental steps")
    m = (rs.rand(N) < 0.5).astype(np.int8)
    m[0] = 1
    env.reset(mask=torch.from_numpy(m))
    ref.v.reset_masked(m)
    check(env, ref, "masked reset")
    rollout(env, ref, 9, tag="after the masked reset")
    for k in range(4):
        env.step()
        ref.step()
        check(env, ref, f"step {k} after the last rollout")


# W = 24: G = 676, the last chunk holds 4 cells; W = 8: G = 100, 4 cells; W = 10: G = 144 and W = 6: G = 64, whole chunks
@pytest.mark.parametrize("W", [24, 10, 6, 8])
def test_tail_chunk_and_its_neighbours(T, W):
    """Both players start on the last row, at every column, and move down without autoreset: the heads land on the border
    row, in and beside the plane's last chunk, and the envs are finished.  The rollout after finds the chunks marked and
    its first step restarts every env, which stores them; what follows a plane in memory must be untouched."""
    N = 130
    env, ref = make(T, N, W, seed=57, rank=1)
    i = np.arange(N)
    sp = np.stack([np.full(N, W - 1), i % W, np.full(N, W - 1), (i + W // 2) % W], 1).astype(np.int8)
    env.reset(start_pos=torch.from_numpy(sp))
    ref.v.set_starts(sp)
    acts = np.full((N, 2), DOWN, np.int8)
    _, reward, done, winner = env.step(torch.from_numpy(acts), autoreset=False)
    _, d, w, r = ref.v.step(acts, autoreset=False, want_obs=False)
    assert np.array_equal(np_(done), d) and np.array_equal(np_(winner), w) and np.array_equal(np_(reward), r)
    assert (d == 1).all()
    G, last = (W + 2) ** 2, ((W + 2) ** 2 - 1) // 16 * 16
    assert (ref.v.grid[:, last:] != -1).any(), "a head must stand in the last chunk"
    check(env, ref, "heads on the border row")
    for K in (1, 64, 65):
        rollout(env, ref, K, tag=f"W={W}")
        o, want = np_(env.obs).reshape(N, 2 * G), ref.obs().reshape(N, 2 * G)
        assert np.array_equal(o[:, G - 1:G + 1], want[:, G - 1:G + 1]), "plane 1's last cell, plane 2's first"
        assert np.array_equal(o[1:, 0], want[1:, 0]) and np.array_equal(o[:, -1], want[:, -1]), "the next env's first byte"


@pytest.mark.parametrize("W", [6, 24])
def test_nibble_space_swap(T, W):
    """A buffer built through the API's writers (starts at every cell parity, three steps of scripted actions without
    autoreset) in which each of the six codes stands in both halves of a chunk and at both nibble positions of a packed
    byte; then one step of the rollout, and a few more, with both planes compared."""
    N = 256
    env, ref = make(T, N, W, seed=77, rank=4)
    rs = np.random.RandomState(W)
    sp = rs.randint(1, W - 1, (N, 4)).astype(np.int8)
    clash = (sp[:, 0] == sp[:, 2]) & (sp[:, 1] == sp[:, 3])
    sp[clash, 3] = sp[clash, 1] % (W - 2) + 1
    env.reset(start_pos=torch.from_numpy(sp))
    ref.v.set_starts(sp)
    for _ in range(3):
        acts = rs.randint(0, 4, (N, 2)).astype(np.int8)
        env.step(torch.from_numpy(acts), autoreset=False)
        ref.v.step(acts, autoreset=False, want_obs=False)
    check(env, ref, "the hand-built boards")
    p1 = ref.obs()[:, 0]
    cell = np.arange(p1.shape[1])
    for code in CODES:
        for half in (0, 1):
            for nib in (0, 1):
                at = ((cell % 16) // 8 == half) & (cell % 2 == nib)
                assert (p1[:, at] == code).any(), f"code {code} is missing in half {half}, nibble {nib}"
    for K in (1, 1, 5):
        rollout(env, ref, K, tag=f"W={W}")
