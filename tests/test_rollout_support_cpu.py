"""rollout_support.Ref, the oracle reference of the GPU rollout tests, on the CPU alone: that its two ways of restarting
leave the same oracle, that its totals and its launch log are what a direct count gives, and that its event counters are
live.  130 envs on a 4x4 board (a restart nearly every step) and 65 on a 10x10 one, 20 steps; every sequence begins with
steps without autoreset, so that finished envs enter the first step that restarts."""
import numpy as np
import pytest

import oracle
from rollout_support import LAUNCH, ORACLE_KEYS, Ref, oracle_obs, tally

SHAPES = [(130, 4), (65, 10)]
STEPS = 20
SEED, RANK = 7, 1
PRE = ("steps_noreset", 3)

# border deaths, same-cell draws and episodes of >= 20 steps that the Ref of test_gpu_rollout_wave.py counted, before that
# class moved to rollout_support, from a fresh reset with seed 7, rank 1: (N, W, nonreversing, steps) -> counts.  A 4x4 game
# has 16 cells and ends within 7 steps, and in 20 steps on 10x10 an episode of 20 must begin at the reset and end in the
# last step, so the third counter is checked on that file's own long case (test_long_episodes: 200 envs, 24x24, 130 steps).
EVENTS = {(130, 4, False, 20): (1111, 75, 0), (130, 4, True, 20): (1165, 69, 0),
          (65, 10, False, 20): (195, 5, 0), (65, 10, True, 20): (246, 10, 0),
          (200, 24, True, 130): (1597, 24, 42)}


@pytest.mark.parametrize("nonrev", [False, True])
@pytest.mark.parametrize("fair", [False, True])
@pytest.mark.parametrize("N,W", SHAPES)
def test_both_restart_forms_agree(N, W, fair, nonrev):
    """step(autoreset=True) against step(autoreset=False) + reset_masked(done): the two paths of Ref.step, and the two
    calls of VecOracle themselves; state, records and totals after every step."""
    a = Ref(oracle, N, W, SEED, RANK, fair=fair)
    b = Ref(oracle, N, W, SEED, RANK, fair=fair, events=True)
    raw = oracle.VecOracle(N, W, seed=SEED, stream=RANK, fair=fair)
    raw.reset_all()
    for r in (a, b):
        r.apply(PRE, nonrev)
    for _ in range(PRE[1]):
        raw.step(autoreset=False, want_obs=False, nonreversing=nonrev)
    assert (a.v.done == 1).any() and (a.v.done == 0).any()       # finished envs enter the first step that restarts
    for s in range(STEPS):
        ra = a.step(nonrev=nonrev)
        rb = b.step(nonrev=nonrev)
        _, d, w, r = raw.step(autoreset=False, want_obs=False, nonreversing=nonrev)
        raw.reset_masked(d == 1)
        for i, name in enumerate(("done", "winner", "reward")):
            assert np.array_equal(ra[i], rb[i]) and np.array_equal(ra[i], (d, w, r)[i]), (s, name)
        sa, sb = a.snapshot(copy=False), b.snapshot(copy=False)
        for k in ORACLE_KEYS + ("totals",):
            assert np.array_equal(sa[k], sb[k]), (s, k)
        for k in ORACLE_KEYS[1:]:
            assert np.array_equal(sa[k], getattr(raw, k)), (s, k, "VecOracle")
        assert np.array_equal(sa["obs"], oracle_obs(oracle, raw.grid)), (s, "obs")
    assert int(a.v.episode.min()) > 0 or W > 4                   # every 4x4 env restarted
    assert a.restarts_per_step == b.restarts_per_step and sum(a.restarts_per_step) > N


@pytest.mark.parametrize("events", [False, True])
@pytest.mark.parametrize("N,W", SHAPES)
def test_totals_match_a_direct_count(N, W, events):
    ref = Ref(oracle, N, W, SEED, RANK, events=events)
    ref.apply(PRE)
    assert not ref.totals.any()                                  # steps outside a rollout are not counted
    entered = ref.v.done == 1
    assert entered.any()
    steps = p1 = p2 = draws = 0
    for s in range(STEPS):
        was_done = ref.v.done == 1
        d, w, _ = ref.step()
        assert np.array_equal(was_done, entered if s == 0 else np.zeros(N, bool))
        assert (d[was_done] == 1).all()                          # a finished env reports done in the step that restarts it
        for e in range(N):
            if not was_done[e]:
                steps += 1
                p1 += d[e] == 1 and w[e] == 1
                p2 += d[e] == 1 and w[e] == 2
                draws += d[e] == 1 and w[e] == 0
    assert list(ref.totals) == [steps, p1, p2, draws]
    assert steps == N * STEPS - int(entered.sum()) and p1 > 0 and p2 > 0 and draws > 0
    d = np.array([1, 1, 0, 1], np.int8)
    assert list(tally(d, np.array([1, 2, 0, 0], np.int8), np.array([True, False, True, True]))) == [3, 1, 0, 1]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("N,W", SHAPES)
def test_launch_log_is_consistent(N, W, K):
    ref = Ref(oracle, N, W, SEED, RANK, at_launch=lambda r: r.v.tick.copy())
    ref.apply(PRE)
    was_done = ref.v.done == 1
    entered = int(was_done.sum())
    tick0 = ref.v.tick.copy()
    ref.roll(K)
    lengths = [len(hit) for _, hit in ref.launches]
    assert lengths == [LAUNCH] * (K // LAUNCH) + ([K % LAUNCH] if K % LAUNCH else [])
    befores = [before for before, _ in ref.launches] + [ref.v.episode]
    for i, (before, hit) in enumerate(ref.launches):
        assert hit.shape == (lengths[i], N) and hit.dtype == bool
        assert np.array_equal(hit.sum(0), befores[i + 1] - befores[i]), i     # restarts in the launch: episode after - before
    assert ref.entered_done == entered and entered > 0           # (autoreset: only the first launch finds finished envs)
    assert ref.launches[0][1][0][was_done].all()                 # ... and restarts them in its first step
    assert len(ref.launch_notes) == len(ref.launches) and np.array_equal(ref.launch_notes[0], tick0)
    assert ref.restarts_per_step == [int(h.sum()) for _, hit in ref.launches for h in hit]
    assert int(ref.totals[0]) == N * K - entered


@pytest.mark.parametrize("N,W,nonrev,steps", list(EVENTS))
def test_event_counters_stay_live(N, W, nonrev, steps):
    ref = Ref(oracle, N, W, SEED, RANK, events=True)
    for _ in range(steps):
        ref.step(nonrev=nonrev)
    assert (ref.border_deaths, ref.same_cell, ref.long_episodes) == EVENTS[(N, W, nonrev, steps)]
    if W == 4:
        assert ref.border_deaths > 0 and ref.same_cell > 0
    if steps > STEPS:
        assert ref.long_episodes > 0
    plain = Ref(oracle, N, W, SEED, RANK)                        # without `events` nothing is counted, and nothing else differs
    for _ in range(steps):
        plain.step(nonrev=nonrev)
    assert (plain.border_deaths, plain.same_cell, plain.long_episodes) == (0, 0, 0)
    assert np.array_equal(plain.totals, ref.totals) and np.array_equal(plain.v.grid, ref.v.grid)
