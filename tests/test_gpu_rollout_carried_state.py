"""k_obs_roll's step loop carries an env's state decoded in registers (heads, cells, alive / done / winner, last actions,
eplen, tick), packs st4 once in the epilogue and writes the four cells of a move as masked ORs on their dwords.  Everything a
caller can read back is compared, exactly, with the C oracle driven the same way (rollout_support.Ref), the records with the
oracle's step by step.  Every case also counts, from the oracle alone, the events it is there for and fails on a count of 0.

Shapes: side 4 with 130 envs (two full waves and a ragged one; heads that share a byte and a dword, head-ons, swap-throughs,
moves off the board), side 24 with 257, side 30 with 65 (cpe 64: bit 63 of the masks).  Launch lengths 1, 7, 8, 9, 64 and
65 + 7: the epilogue's pack after a move, after a restart in the launch's last step, and with envs that entered finished.
"""
import numpy as np
import pytest

from rollout_support import Ref, apply, check_against_oracle, gpu_modules, make_tape, new_totals, pull

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, RANK = 0xC0DE, 3
SHAPES = [(4, 130), (24, 257), (30, 65)]
LENS = (1, 7, 8, 9, 64, 65 + 7)


@pytest.fixture(scope="module")
def mods():
    return gpu_modules()


def pair(mods, W, N, **kw):
    tv, oracle = mods
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes")
    env.reset()
    return env, new_totals(), Ref(oracle, N, W, SEED, RANK, **kw)


def run_ops(mods, W, N, ops, nonrev=False, **kw):
    env, totals, ref = pair(mods, W, N, **kw)
    for i, op in enumerate(ops):
        apply(env, totals, op, nonrev)
        ref.apply(op, nonrev)
        check_against_oracle(pull(env, totals), ref, (W, N, i, op))
    env.close()
    return ref


def last_step_restarts(ref):
    return sum(int(hit[-1].sum()) for _, hit in ref.launches)


# ---- the launch lengths: two launches each, so the second enters by what the first one's epilogue packed
@pytest.mark.parametrize("K", LENS)
@pytest.mark.parametrize("W,N", SHAPES)
def test_launch_lengths(mods, W, N, K):
    ref = run_ops(mods, W, N, [("steps", 5), ("roll", K), ("roll", K)], events=True)
    if W == 4:                                                   # a 4x4 game lasts at most 7 steps: every step restarts some env
        assert last_step_restarts(ref) > 0
        if K >= 64:
            assert ref.border_deaths > 0 and ref.same_cell > 0
    elif K >= 64:
        assert last_step_restarts(ref) > 0


# ---- st4 through memory: rollout, per-step launches, rollout (a full-read entry behind a masked one)
@pytest.mark.parametrize("W,N", SHAPES)
def test_st4_round_trip(mods, W, N):
    ref = run_ops(mods, W, N, [("roll", 9), ("roll", 8), ("steps", 3), ("roll", 65 + 7), ("steps", 1), ("roll", 7)])
    assert sum(int(hit.sum()) for _, hit in ref.launches) > 0    # restarts inside the launches


# ---- envs that enter a launch finished: a launch of one step is then a launch in which such an env never moves
@pytest.mark.parametrize("W,N,pre", [(4, 130, 2), (24, 257, 2), (30, 65, 2)])
def test_finished_entries(mods, W, N, pre):
    ref = run_ops(mods, W, N, [("steps_noreset", pre), ("roll", 1), ("steps_noreset", pre), ("roll", 9)])
    assert ref.entered_done > 0
    assert any(int((~hit[0]).sum()) > 0 for _, hit in ref.launches)          # and envs that entered live beside them


# ---- the non-reversing policy: the carried last actions across a launch boundary and a restart (last == 0 behind it)
@pytest.mark.parametrize("W,N", SHAPES[:2])
def test_nonreversing(mods, W, N):
    ref = run_ops(mods, W, N, [("roll", 7), ("roll", 65 + 7), ("steps", 2), ("roll", 9), ("roll", 64)], nonrev=True)
    assert len(ref.launches) == 5
    assert sum(int(hit[:-1].sum()) for _, hit in ref.launches) > 0           # a restart with steps of the launch behind it


# ---- tapes: rollout_actions with and without records, the reward table that pays the step index (the carried eplen)
def cells_of(pos, S):
    p = pos.astype(np.int64)
    return np.stack([(p[:, 0] + 1) * S + p[:, 1] + 1, (p[:, 2] + 1) * S + p[:, 3] + 1], 1)


def play_tape(mods, W, N, tape, records, reward_tape):
    """The env through rollout_actions, the oracle through the same rows step by step; returns what the oracle counted:
    (env-steps whose four cells share a byte, a dword; new heads that land in a chunk an earlier game of the launch left)."""
    tv, oracle = mods
    env = tv.VecTron(N, W, seed=SEED, rank=RANK, obs_format="codes")
    env.set_reward(**oracle.REWARD_DQN)
    env.reset()
    totals = new_totals()
    ref = Ref(oracle, N, W, SEED, RANK, reward=oracle.REWARD_DQN)
    K, S = tape.shape[0], W + 2
    rec = None
    if records:
        rec = (torch.empty(K, N, 2, device="cuda") if reward_tape else None,
               torch.empty(K, N, dtype=torch.int8, device="cuda"), torch.empty(K, N, dtype=torch.int8, device="cuda"))
    env.rollout_actions(tape, totals, records=rec)
    host = tape.cpu().numpy()
    rows = []
    byte = dword = stale_heads = 0
    stale = np.zeros((N, (S * S + 15) // 16), bool)
    for k in range(K):
        if k % 64 == 0:
            stale[:] = False                                     # (an entry's own stale chunks are not counted: a lower bound)
        old, ep = cells_of(ref.v.pos, S), ref.v.episode.copy()
        rows.append(ref.step(actions=host[k]))
        new, hit = cells_of(ref.v.pos, S), ref.v.episode != ep
        four = np.concatenate([old, new], 1)[~hit]
        q1, q3 = np.sort(four >> 1, 1), np.sort(four >> 3, 1)
        byte += int((q1[:, 1:] == q1[:, :-1]).any(1).sum())
        dword += int((q3[:, 1:] == q3[:, :-1]).any(1).sum())
        e = np.nonzero(~hit)[0]
        for p in range(2):
            stale_heads += int(stale[e, new[e, p] >> 4].sum())
            stale[e, new[e, p] >> 4] = False
        stale[hit] = True
        for p in range(2):
            stale[np.nonzero(hit)[0], new[hit, p] >> 4] = False
    check_against_oracle(pull(env, totals), ref, (W, N, K, records, reward_tape))
    if records:
        d, w, r = (np.stack([np.asarray(row[i]) for row in rows]) for i in range(3))
        assert np.array_equal(rec[1].cpu().numpy(), d.astype(np.int8)) and np.array_equal(rec[2].cpu().numpy(), w.astype(np.int8))
        if reward_tape:
            assert np.array_equal(rec[0].cpu().numpy().view(np.uint32), r.astype(np.float32).view(np.uint32))
            assert len(np.unique(r[d == 0])) > 2                 # the step index is paid: eplen is live
    env.close()
    return byte, dword, stale_heads


@pytest.mark.parametrize("records,reward_tape", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("W,N", SHAPES)
def test_tapes(mods, W, N, records, reward_tape):
    byte, dword, stale_heads = play_tape(mods, W, N, make_tape(N, 65 + 7, salt=W), records, reward_tape)
    assert dword > 0 and stale_heads > 0
    if W == 4:
        assert byte > 0


# ---- the masked ORs: both players kept on cells of one dword (a 4x4 board's row is six cells, a dword eight), step after step
def test_heads_of_one_dword(mods):
    W, N, K = 4, 130, 65 + 7
    one = make_tape(N, K, salt=77)
    tape = one[:, :, :1].expand(K, N, 2).contiguous()            # both players take the same heading: they stay side by side
    byte, dword, stale_heads = play_tape(mods, W, N, tape, True, True)
    assert byte > N and dword > 4 * N and stale_heads > 0
