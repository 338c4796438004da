"""On the oracle alone: the inputs of tests/test_gpu_rollout_cell_space.py (same seed, stream, shapes and step counts) reach
every path the cell-space step loop added, each at least FLOOR times.

An env is called OWED here from a restart inside a launch until its next move that is written — a move that does not end
its game — or the launch's end: the span in which its heads come from rs4.nstart and not from a move, which is where the
cell-space state (cells set by a restart, moved by a delta byte, divided back into r and c by the epilogue) and a restart
that defers its board writes can go wrong.  A launch is at most 64 steps of one call; the calls are 1, 2, 7, 8, 9, 64, 65 and 72 steps (the one-step
call is a per-step launch and is not counted as a launch here).
"""
import numpy as np
import pytest

from rollout_support import LAUNCH, Ref

SEED, RANK = 0xE7A5, 3                                           # test_gpu_rollout_entry_masks', whose run_sequence the GPU file runs
LENS = (1, 2, 7, 8, 9, 64, 65, 72)
SHAPES = [(4, 63, True), (4, 257, False), (6, 64, True), (6, 257, False), (24, 257, False), (30, 257, False)]
FLOOR = 8


def cells(pos, S):
    p = pos.astype(np.int64)
    return np.stack([(p[:, 0] + 1) * S + p[:, 1] + 1, (p[:, 2] + 1) * S + p[:, 3] + 1], 1)


def count(oracle, W, N, fair, nonrev=False):
    S, G = W + 2, (W + 2) * (W + 2)
    short = (G + 15) // 16 - 1 if G % 16 else -1                 # the short last chunk, if the board has one
    seen = {}

    def keep(ref, fin):
        seen["pos"] = ref.v.pos.copy()                           # the finished boards' heads, before the restart moves them

    ref = Ref(oracle, N, W, SEED, RANK, fair=fair, before_restart=keep)
    v = ref.v
    c = dict(owed_at_epilogue=0, owed_dies=0, owed_dies_twice=0, starts_one_chunk=0, starts_one_dword=0, into_start_cell=0,
             head_on=0, up=0, down=0, left=0, right=0, short_chunk=0, first_same_chunk=0, first_other_chunk=0)
    owed = np.zeros(N, bool)
    died_owed = np.zeros(N, bool)                                # the env's last game ended on its first move, owed
    for K in LENS:
        for k0 in range(0, K, LAUNCH):
            k = min(K - k0, LAUNCH)
            owed[:] = False                                      # a launch's epilogue materialises; a per-step launch owes nothing
            for s in range(k):
                old, first = cells(v.pos, S), v.eplen == 0
                seen.pop("pos", None)
                d, _, _ = ref.step(nonrev=nonrev)
                fin = d == 1
                pos = seen.get("pos", v.pos)
                new = cells(pos, S)
                p = pos.astype(np.int64)
                # the moves (every env moves: all are live under autoreset)
                c["head_on"] += int((new[:, 0] == new[:, 1]).sum())
                c["into_start_cell"] += int((first & ((new[:, 0] == old[:, 1]) | (new[:, 1] == old[:, 0]))).sum())
                for q in (0, 2):
                    c["up"] += int((fin & (p[:, q] == -1)).sum())
                    c["down"] += int((fin & (p[:, q] == W)).sum())
                    c["left"] += int((fin & (p[:, q + 1] == -1)).sum())
                    c["right"] += int((fin & (p[:, q + 1] == W)).sum())
                c["short_chunk"] += int((fin[:, None] & ((new >> 4) == short)).any(1).sum())
                if K >= 2:
                    dies = owed & fin                            # (owed implies the game's first move)
                    c["owed_dies"] += int(dies.sum())
                    c["owed_dies_twice"] += int((dies & died_owed).sum())
                    died_owed = dies
                    wrote = owed & ~fin
                    same = (old >> 4) == (new >> 4)
                    c["first_same_chunk"] += int((wrote[:, None] & same).sum())
                    c["first_other_chunk"] += int((wrote[:, None] & ~same).sum())
                    owed = fin.copy()                            # restarted in this step, nothing written since
                    st = cells(v.pos, S)[fin]                    # the restarted envs' start heads
                    c["starts_one_chunk"] += int(((st[:, 0] >> 4) == (st[:, 1] >> 4)).sum())
                    c["starts_one_dword"] += int(((st[:, 0] >> 3) == (st[:, 1] >> 3)).sum())
            if K >= 2:
                c["owed_at_epilogue"] += int(owed.sum())
    return c, short >= 0


@pytest.fixture(scope="module")
def oracle():
    import oracle
    return oracle


@pytest.mark.parametrize("W,N,fair", SHAPES)
def test_inputs_reach_the_new_paths(oracle, W, N, fair):
    c, has_short = count(oracle, W, N, fair)
    for k, n in c.items():
        print(f"side {W}, {N} envs, fair {fair}: {k} {n}")
    for k, n in c.items():
        if k == "short_chunk" and not has_short:
            continue                                             # (sides 6 and 30: the last chunk is a whole one)
        assert n >= FLOOR, (W, N, fair, k, n)


def test_the_nonreversing_policy_reaches_them_too(oracle):
    c, _ = count(oracle, 4, 257, False, nonrev=True)
    for k in ("owed_at_epilogue", "owed_dies", "owed_dies_twice", "head_on", "first_same_chunk", "first_other_chunk"):
        assert c[k] >= FLOOR, (k, c[k])
