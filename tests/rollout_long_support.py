"""What tests/test_gpu_rollout_long_launch.py and tests/test_rollout_long_launch_cpu.py share: the cases (shapes, seeds,
sequences of calls) and the oracle's side of a sequence, with the launches a call of the roll_resident family makes now —
the whole call, up to CAP steps (ROLL_LAUNCH_CAP in csrc/tron_env.hip); a longer call as launches of CAP, the remainder
last — and, per launch, which env restarted, finished and won in which step.  A plain module like rollout_support.py;
nothing here touches the GPU."""
import numpy as np

from rollout_support import Ref

CAP = 1024                                                       # steps per launch at the most (ROLL_LAUNCH_CAP)
OLD = 64                                                         # the launches of the TRON_ROLL_CHUNK=64 twin (TRON_ROLLOUT_CHUNK)
FLUSH = 128                                                      # steps between two flushes of the per-lane byte tallies
R = 8                                                            # steps per block (ROLL_R); the start ring holds 2 R ordinals
SEED, RANK = 0x10A6, 3
FOLLOW_MAX = 64                                                  # per-step launches behind a sequence, at the most
# past the old boundary, around both tally flushes, at the cap, one step and one block past it
STEPS = (65, 72, 127, 128, 129, 136, 255, 256, 257, 320, 1024, 1025, 1032)
SIDES = (4, 24, 30)
ENVS = (1, 64, 65, 257, 16384 + 1)


def all_kernels(K):
    """One call of K steps per instantiation (k_obs_roll with either policy, k_obs_roll_tape, k_obs_roll_tape_rec): every
    call but the first enters handed, behind a long launch."""
    return [("roll", K, False), ("tape", K), ("rec", K), ("roll", K, True)]


# name -> (N, W, fair, ops).  ops: ("roll", K, non-reversing policy) | ("tape", K) | ("rec", K): a tape with records |
# ("rec_rows", K, r0, r1): rows r0..r1 of a K-row tape whose salt is K, with records | ("steps", n) | ("steps_noreset", n) |
# ("survive", K): survive_tape's K rows, the first op of its case
CASES = {}
for _W in SIDES:
    for _K in STEPS:                                             # (fair at side 4 here, off at side 4 in the sequences below)
        CASES[f"steps-{_K}-{_W}"] = (257, _W, _W == 4, all_kernels(_K))
for _W, _f in ((4, False), (4, True), (24, False), (24, True), (30, False)):
    for _N in ENVS[:3]:
        CASES[f"envs-{_N}-{_W}-{int(_f)}"] = (_N, _W, _f, [("roll", 320, False), ("rec", 136), ("roll", 257, True)])
for _W, _f in ((4, False), (24, True), (30, False)):             # four / three game waves per workgroup
    CASES[f"envs-{ENVS[4]}-{_W}-{int(_f)}"] = (ENVS[4], _W, _f, [("roll", 320, _W == 30), ("tape", 72), ("roll", 129, _W != 30)])
for _W, _f in ((4, False), (24, False), (30, False)):
    for _N in (65, 257):
        CASES[f"long_long-{_W}-{_N}"] = (_N, _W, _f, [("roll", 320, False), ("roll", 257, True), ("roll", 136, False)])
        CASES[f"full_read-{_W}-{_N}"] = (_N, _W, _f, [("roll", 320, True), ("steps", 3), ("roll", 257, False)])
        CASES[f"tape_roll-{_W}-{_N}"] = (_N, _W, _f, [("tape", 200), ("roll", 130, False)])
        CASES[f"split_records-{_W}-{_N}"] = (_N, _W, _f, [("rec_rows", 200, 0, 130), ("rec_rows", 200, 130, 200)])
        CASES[f"finished-{_W}-{_N}"] = (_N, _W, _f, [("steps_noreset", 5), ("roll", 320, False), ("roll", 65, True)])
for _N in (65, 257):                                             # envs that do not restart for 64 steps and more (survive_tape)
    CASES[f"idle-30-{_N}"] = (_N, 30, False, [("survive", 200), ("roll", 130, True)])


def host_tape(N, K, salt):
    """[K, N, 2] int8 in 0..3 on the host (both processes and the CPU file make the same one)."""
    return np.random.RandomState((1_000_003 * N + 131 * K + salt) % 2 ** 32).randint(0, 4, (K, N, 2)).astype(np.int8)


def survive_tape(oracle, N, W, fair, K):
    """[K, N, 2] int8: moves that keep both players of a freshly reset batch alive as long as a look at the four neighbours
    can — straight on while the cell ahead is empty (and not the cell player 1 has just chosen), else a turn.  Random play
    does not leave an env without a restart for 64 steps at any size a test can afford (the non-reversing policy at side
    30: the longest of 430 M env-steps, 1 600 seeds of 257 envs x 1 024 steps, was under 64; a seed's own longest is 35 to
    48), so the launches that need such envs play this tape.  Made on the oracle, the same in every process."""
    ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
    v, S, n = ref.v, W + 2, np.arange(N)
    dr, dc = np.array([-1, 0, 1, 0]), np.array([0, 1, 0, -1])   # UP, RIGHT, DOWN, LEFT
    tape, last = np.zeros((K, N, 2), np.int8), np.zeros((N, 2), np.int64)
    for s in range(K):
        grid, taken = v.grid.reshape(N, S * S), np.full(N, -1)
        for p in range(2):
            r, c = v.pos[:, 2 * p].astype(np.int64) + 1, v.pos[:, 2 * p + 1].astype(np.int64) + 1
            best, found = last[:, p].copy(), np.zeros(N, bool)
            for turn in (0, 1, 3, 2):
                a = (last[:, p] + turn) % 4
                to = (r + dr[a]) * S + c + dc[a]
                ok = (grid[n, to] == 0) & (to != taken) & ~found
                best, found = np.where(ok, a, best), found | ok
            last[:, p] = tape[s, :, p] = best
            taken = (r + dr[best]) * S + c + dc[best]
        ref.step(actions=tape[s])
    return tape


def op_tape(N, op, i, oracle=None, W=0, fair=False):
    """The rows an op plays, or None: a tape of its own (salt: the op's index), a slice of the K-row tape (salt: K), or
    survive_tape's (the case's first op: the batch is freshly reset)."""
    if op[0] == "survive":
        assert i == 0
        return survive_tape(oracle, N, W, fair, op[1])
    if op[0] in ("tape", "rec"):
        return host_tape(N, op[1], i)
    if op[0] == "rec_rows":
        return host_tape(N, op[1], op[1])[op[2]:op[3]]
    return None


def launch_lengths(K, chunk=CAP):
    return [min(chunk, K - k0) for k0 in range(0, K, chunk)]


class Model:
    """A Ref stepped through a sequence.  launches: per launch of the roll_resident family a dict — k, handed (the call
    before it on the handle was such a launch), tape, before ([N] episode at entry), hit / fin ([k, N] bool: restarted /
    finished by a move in step s) and win ([k, N] the finished game's winner)."""

    def __init__(self, oracle, N, W, fair, chunk=CAP):
        self.ref = Ref(oracle, N, W, SEED, RANK, fair=fair)
        self.oracle, self.N, self.W, self.fair, self.chunk, self.handed, self.launches = oracle, N, W, fair, chunk, False, []

    def rollout(self, K, nonrev=False, tape=None):
        """K steps with autoreset; the (done, winner, reward) rows of every step, [K, ...] each."""
        rows = []
        v = self.ref.v
        k0 = 0
        for k in launch_lengths(K, self.chunk):
            before = v.episode.copy()
            hit, fin, win = np.zeros((k, self.N), bool), np.zeros((k, self.N), bool), np.zeros((k, self.N), np.int8)
            for s in range(k):
                ep, live = v.episode.copy(), v.done == 0
                d, w, r = self.ref.step(actions=None if tape is None else tape[k0 + s], nonrev=nonrev)
                rows.append((d.copy(), w.copy(), r.copy()))
                hit[s], fin[s], win[s] = v.episode != ep, (d == 1) & live, w
            self.launches.append(dict(k=k, handed=self.handed, tape=tape is not None, before=before, hit=hit, fin=fin, win=win))
            self.handed = True
            k0 += k
        return tuple(np.stack([r[i] for r in rows]) for i in range(3))

    def op(self, op, i):
        if op[0] in ("roll", "tape", "rec", "rec_rows", "survive"):
            tape = op_tape(self.N, op, i, self.oracle, self.W, self.fair)
            return self.rollout(op[1] if tape is None else len(tape), op[0] == "roll" and op[2], tape)
        self.handed = False
        for _ in range(op[1]):
            self.ref.step(autoreset=op[0] == "steps", count=False)
        return None


def model_case(oracle, name, chunk=CAP):
    N, W, fair, ops = CASES[name]
    mod = Model(oracle, N, W, fair, chunk)
    for i, op in enumerate(ops):
        mod.op(op, i)
    return mod


def longest_idle(hit):
    """[N]: the longest run of consecutive steps of a launch in which the env does not restart."""
    best, run = np.zeros(hit.shape[1], np.int64), np.zeros(hit.shape[1], np.int64)
    for row in hit:
        run = np.where(row, 0, run + 1)
        best = np.maximum(best, run)
    return best


def tally_windows(launch):
    """Per flush window of a launch (FLUSH steps, the last one shorter) the per-env counts the byte tallies hold when they
    are flushed: [windows, 4, N] — steps, player-1 wins, player-2 wins, draws."""
    out = []
    stepped = launch["hit"].copy()                               # an env moves in every step but the one it enters finished in
    stepped[:] = True
    stepped[0] = launch["fin"][0] | ~launch["hit"][0]            # step 0: a restart without a move is no step
    for s0 in range(0, launch["k"], FLUSH):
        sl = slice(s0, min(s0 + FLUSH, launch["k"]))
        f, w = launch["fin"][sl], launch["win"][sl]
        out.append(np.stack([stepped[sl].sum(0), (f & (w == 1)).sum(0), (f & (w == 2)).sum(0), (f & (w == 0)).sum(0)]))
    return np.stack(out)
