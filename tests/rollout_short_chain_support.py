"""What tests/test_gpu_rollout_short_chain.py and tests/test_rollout_short_chain_cpu.py share: the shapes, the sequence of
calls and the oracle-side model that counts, from the oracle alone, the cases the shorter step chain of the roll_resident
family can go wrong at.  A plain module; nothing here touches the GPU.

The sequence.  For each k of KS: a reset (so the first call enters by the full read and draws its own first block), then
three calls of k steps on the one handle (the second and third enter masked and handed: ring slots written by the launch
before are read in cell space).  Then two calls behind per-step steps with autoreset and two behind steps WITHOUT
autoreset (both invalidate the hand-off; behind the latter the launch is entered with finished envs).  A call of one step
is a per-step launch; every longer call is one persistent launch (129 steps cross the 128-step tally flush).
"""
import numpy as np

from rollout_support import Ref

SEED, RANK = 0x31C4, 2
SIDES = (4, 6, 24, 30)
NS = (1, 65, 257)
KS = (1, 2, 7, 8, 9, 20, 129)
KINDS = ("uniform", "nonreversing", "tape", "records")
OPS = []
for _k in KS:
    OPS += [("reset",), ("call", _k), ("call", _k), ("call", _k)]
OPS += [("steps", 2), ("call", 9), ("call", 9), ("steps_noreset", 3), ("call", 9), ("call", 20)]
FOLLOW_MAX = 96                                                  # per-step launches behind a sequence, at the most

COUNTS = ("restarts_0", "restarts_1", "restarts_2_and_more", "restart_in_last_step", "restart_in_first_step_handed",
          "starts_one_chunk", "starts_one_dword", "first_move_leaves_start_chunk", "dead_up", "dead_down", "dead_left",
          "dead_right", "dead_on_short_chunk", "head_in_chunk_63", "entered_finished")


def host_tape(N, K, salt=0):
    """rollout_support.make_tape's [K, N, 2] int8 actions, on the host (the same seeded torch.Generator; the GPU file
    asserts the two equal), so that the oracle alone can play the tape cases."""
    import torch
    g = torch.Generator().manual_seed(1_000_003 * N + 131 * K + salt)
    return torch.randint(0, 4, (K, N, 2), generator=g, dtype=torch.int64).to(torch.int8).numpy()


def cells(pos, S):
    p = pos.astype(np.int64)
    return np.stack([(p[:, 0] + 1) * S + p[:, 1] + 1, (p[:, 2] + 1) * S + p[:, 3] + 1], 1)


class Model:
    """A Ref (DQN's reward table: the step reward is the episode's step index) driven through OPS, the host's hand-off flag
    as the library keeps it (`handed`: the op before was a persistent launch), and the counts."""

    def __init__(self, oracle, N, W, fair, kind):
        self.ref = Ref(oracle, N, W, SEED, RANK, fair=fair, reward=oracle.REWARD_DQN, before_restart=self._keep)
        self.N, self.W, self.S, self.G = N, W, W + 2, (W + 2) * (W + 2)
        self.nonrev = kind == "nonreversing"
        self.short = (self.G + 15) // 16 - 1 if self.G % 16 else -1  # the short last chunk, if the board has one
        self.handed = False
        self.c = dict.fromkeys(COUNTS, 0)
        self._pos = None

    def _keep(self, ref, fin):
        self._pos = ref.v.pos.copy()                                 # the finished boards' heads, before the restart moves them

    def call(self, K, tape=None):
        """K steps with autoreset as one rollout call makes them; the (done, winner, reward) rows of every step."""
        v, c, S, W = self.ref.v, self.c, self.S, self.W
        launch = K >= 2                                              # (a single step is a per-step launch)
        handed = launch and self.handed
        if launch:
            c["entered_finished"] += int((v.done == 1).sum())
        nres = np.zeros(self.N, np.int64)
        rows = []
        for s in range(K):
            old, first, moved = cells(v.pos, S), v.eplen == 0, v.done == 0
            self._pos = None
            rows.append(self.ref.step(actions=None if tape is None else tape[s], nonrev=self.nonrev))
            if not launch:
                continue
            fin = rows[-1][0] == 1
            pos = v.pos if self._pos is None else self._pos
            new, p = cells(pos, S), pos.astype(np.int64)
            nres += fin
            c["first_move_leaves_start_chunk"] += int((moved & first & ((old >> 4) != (new >> 4)).any(1)).sum())
            dead = fin & moved
            for q in (0, 2):
                c["dead_up"] += int((dead & (p[:, q] == -1)).sum())
                c["dead_down"] += int((dead & (p[:, q] == W)).sum())
                c["dead_left"] += int((dead & (p[:, q + 1] == -1)).sum())
                c["dead_right"] += int((dead & (p[:, q + 1] == W)).sum())
            c["dead_on_short_chunk"] += int((dead[:, None] & ((new >> 4) == self.short)).any(1).sum())
            c["head_in_chunk_63"] += int((dead[:, None] & ((new >> 4) == 63)).any(1).sum())
            st = cells(v.pos, S)[fin]                                # the restarted envs' start heads
            c["starts_one_chunk"] += int(((st[:, 0] >> 4) == (st[:, 1] >> 4)).sum())
            c["starts_one_dword"] += int(((st[:, 0] >> 3) == (st[:, 1] >> 3)).sum())
            if s == K - 1:
                c["restart_in_last_step"] += int(fin.sum())
            if s == 0 and handed:
                c["restart_in_first_step_handed"] += int(fin.sum())
        if launch:
            c["restarts_0"] += int((nres == 0).sum())
            c["restarts_1"] += int((nres == 1).sum())
            c["restarts_2_and_more"] += int((nres >= 2).sum())
        self.handed = launch
        return tuple(np.stack([r[i] for r in rows]) for i in range(3))

    def op(self, op, tape=None):
        if op[0] == "call":
            return self.call(op[1], tape)
        self.handed = False
        if op[0] == "reset":
            self.ref.v.reset_all()
        else:
            for _ in range(op[1]):
                self.ref.step(nonrev=self.nonrev, autoreset=op[0] == "steps", count=False)
        return None

    def can_occur(self, name):
        """Whether a count can be above 0 at this side at all."""
        if name == "dead_on_short_chunk":
            return self.short >= 0
        if name == "head_in_chunk_63":
            return self.G > 63 * 16
        return True
