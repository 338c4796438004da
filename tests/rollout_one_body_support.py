"""What tests/test_gpu_rollout_one_body.py and tests/test_rollout_one_body_cpu.py share: the shapes, the sequence of calls
(rollout_short_chain_support's, under another seed and stream) and an oracle-side model that keeps, per env, the chunk
sets the one step body of the roll_resident family keeps — mask (chunks that differ from the fresh board) and stale
(chunks whose LDS bytes are a finished game's trail) — and counts the cases that body can go wrong at.  A plain module;
nothing here touches the GPU.

The chunk sets follow the kernel's rules: a launch behind another launch is entered masked (stale = every chunk outside
the mask the launch before left), any other launch by the full read (mask = the chunks that differ, stale empty); a move
that does not finish refreshes and marks its two new head chunks; a restart — in the step its game finishes in, or in a
launch's first step for an env that entered finished — turns the mask stale and marks its two start chunks.
"""
import numpy as np

from rollout_short_chain_support import FOLLOW_MAX, KINDS, KS, NS, SIDES, Model as ShortChainModel, cells, host_tape  # noqa: F401
from rollout_short_chain_support import OPS
from rollout_support import WALL, Ref

EMPTY = 1                                                        # raw tile value of a free cell (map.py:9-17)

SEED, RANK = 0x34B0D1, 3
# behind the shared sequence: a reset and one launch of a tape whose first row is safe for every env (safe_tape), so that a
# whole wave is on the move path with no lane restarting, then an ordinary tape call behind it (masked, handed)
OPS = OPS + [("reset",), ("safe", 2), ("call", 7)]

COUNTS = ("restart_start_in_old_trail", "starts_one_chunk", "starts_one_dword", "move_into_stale_chunk_after_restart",
          "both_new_heads_in_one_stale_chunk", "game_ends_in_first_move_after_restart", "restart_in_last_step",
          "restart_in_first_step_handed", "entered_finished", "restart_without_move", "step_all_move_none_restarts",
          "step_every_env_restarts", "dead_up", "dead_down", "dead_left", "dead_right", "dead_on_short_chunk",
          "dead_in_chunk_63", "start_in_short_chunk", "start_in_chunk_63", "entered_finished_handed")
# Start cells are cells of the board proper; the short last chunk (sides 4 and 24) and chunk 63 (side 30) are cells of the
# border's last row, and the hand-off is taken only behind a launch with autoreset, which leaves no env finished.
NEVER = ("start_in_short_chunk", "start_in_chunk_63", "entered_finished_handed")


DR, DC = (-1, 0, 1, 0), (0, 1, 0, -1)                           # actions 0 .. 3: up, right, down, left (cell_deltas)


def safe_tape(pos, W, K, salt):
    """[K, N, 2] int8 actions for boards that hold nothing but the two heads (behind a reset; pos is state()'s [N, 4]): row 0
    moves both players of every env onto free cells of the board, two different ones, so no game ends in the launch's
    first step; the other rows are host_tape's."""
    p = np.asarray(pos).astype(np.int64)
    N = len(p)
    tape = host_tape(N, K, salt=salt).copy()
    found = np.zeros(N, bool)
    for a0 in range(4):
        for a1 in range(4):
            r0, c0, r1, c1 = p[:, 0] + DR[a0], p[:, 1] + DC[a0], p[:, 2] + DR[a1], p[:, 3] + DC[a1]
            ok = (r0 >= 0) & (r0 < W) & (c0 >= 0) & (c0 < W) & (r1 >= 0) & (r1 < W) & (c1 >= 0) & (c1 < W)
            ok &= ~((r0 == p[:, 2]) & (c0 == p[:, 3])) & ~((r1 == p[:, 0]) & (c1 == p[:, 1])) & ~((r0 == r1) & (c0 == c1))
            take = ok & ~found
            tape[0, take, 0], tape[0, take, 1] = a0, a1
            found |= ok
    assert found.all()
    return tape


class Model(ShortChainModel):
    def __init__(self, oracle, N, W, fair, kind):
        super().__init__(oracle, N, W, fair, kind)
        self.ref = Ref(oracle, N, W, SEED, RANK, fair=fair, reward=oracle.REWARD_DQN, before_restart=self._keep)   # (this file's seed)
        self.C = (self.G + 15) // 16
        self.c = dict.fromkeys(COUNTS, 0)
        self.mask = np.zeros((N, self.C), bool)
        self.stale = np.zeros((N, self.C), bool)

    def differs(self):
        """[N, C]: the chunks of every env's board that differ from the fresh board (border wall, empty inside)."""
        g = np.asarray(self.ref.v.grid).reshape(self.N, self.S, self.S)
        inner = np.zeros((self.S, self.S), bool)
        inner[1:-1, 1:-1] = True
        d = np.where(inner[None], g != EMPTY, g != WALL).reshape(self.N, self.G)
        pad = np.zeros((self.N, self.C * 16), bool)
        pad[:, :self.G] = d
        return pad.reshape(self.N, self.C, 16).any(2)

    def call(self, K, tape=None):
        v, c, S, W, N = self.ref.v, self.c, self.S, self.W, self.N
        launch = K >= 2                                              # (a single step is a per-step launch)
        handed = launch and self.handed
        ar = np.arange(N)
        if launch:
            c["entered_finished"] += int((v.done == 1).sum())
            if handed:
                c["entered_finished_handed"] += int((v.done == 1).sum())
                self.stale = ~self.mask
            else:
                self.mask = self.differs()
                self.stale = np.zeros_like(self.mask)
        just = np.zeros(N, bool)                                     # restarted in the step before, in this launch
        rows = []
        for s in range(K):
            first, moved = v.eplen == 0, v.done == 0
            self._pos = None
            rows.append(self.ref.step(actions=None if tape is None else tape[s], nonrev=self.nonrev))
            if not launch:
                continue
            fin = rows[-1][0] == 1
            pos = v.pos if self._pos is None else self._pos          # the heads the move left, a finished game's included
            new, p = cells(pos, S), pos.astype(np.int64)
            nk = new >> 4
            go = moved & ~fin                                        # the move's board work
            st0, st1 = self.stale[ar, np.minimum(nk[:, 0], self.C - 1)], self.stale[ar, np.minimum(nk[:, 1], self.C - 1)]
            c["move_into_stale_chunk_after_restart"] += int((go & first & just & (st0 | st1)).sum())
            c["both_new_heads_in_one_stale_chunk"] += int((go & (nk[:, 0] == nk[:, 1]) & st0).sum())
            c["game_ends_in_first_move_after_restart"] += int((moved & fin & first & just).sum())
            for q in (0, 1):
                e = ar[go]
                self.stale[e, nk[go, q]] = False
                self.mask[e, nk[go, q]] = True
            dead = fin & moved
            for q in (0, 2):
                c["dead_up"] += int((dead & (p[:, q] == -1)).sum())
                c["dead_down"] += int((dead & (p[:, q] == W)).sum())
                c["dead_left"] += int((dead & (p[:, q + 1] == -1)).sum())
                c["dead_right"] += int((dead & (p[:, q + 1] == W)).sum())
            c["dead_on_short_chunk"] += int((dead[:, None] & (nk == self.short)).any(1).sum())
            c["dead_in_chunk_63"] += int((dead[:, None] & (nk == 63)).any(1).sum())
            # the restarts: the start heads are the oracle's after its reset
            stc = cells(v.pos, S)
            sk = stc >> 4
            e = ar[fin]
            c["restart_start_in_old_trail"] += int((self.mask[e, sk[fin, 0]] | self.mask[e, sk[fin, 1]]).sum())
            c["starts_one_chunk"] += int((sk[fin, 0] == sk[fin, 1]).sum())
            c["starts_one_dword"] += int(((stc[fin, 0] >> 3) == (stc[fin, 1] >> 3)).sum())
            c["start_in_short_chunk"] += int((sk[fin] == self.short).any(1).sum())
            c["start_in_chunk_63"] += int((sk[fin] == 63).any(1).sum())
            c["restart_without_move"] += int((fin & ~moved).sum())
            self.stale[fin] |= self.mask[fin]
            self.mask[fin] = False
            for q in (0, 1):
                self.stale[e, sk[fin, q]] = False
                self.mask[e, sk[fin, q]] = True
            if s == K - 1:
                c["restart_in_last_step"] += int(fin.sum())
            if s == 0 and handed:
                c["restart_in_first_step_handed"] += int(fin.sum())
            lanes = min(N, 64)                                       # the first wave
            c["step_all_move_none_restarts"] += int(moved[:lanes].all() and not fin[:lanes].any())
            c["step_every_env_restarts"] += int(fin.all())
            just = fin
        self.handed = launch
        return tuple(np.stack([r[i] for r in rows]) for i in range(3))

    def op(self, op, tape=None):
        if op[0] == "safe":
            return self.call(op[1], tape)
        return super().op(op, tape)

    def can_occur(self, name):
        if name in NEVER:
            return False
        if name == "dead_on_short_chunk":
            return self.short >= 0
        if name == "dead_in_chunk_63":
            return self.G > 63 * 16
        if name == "step_every_env_restarts":
            return self.N == 1                                       # (asked of the one-env wave)
        return True
