"""What the sliding-playout tests share (tests/test_playout_slide_model_cpu.py, tests/test_gpu_playout_slide.py): the host
model of tron_playout_slide_codes and the inputs both files use.  The model is playout_support.Playouts on a VecOracle in
mode "ice" whose every env slides at 0.5: per step it decides `float64(u) <= rate` per (playout, player) in numpy and
hands orc_step the uniform 0.25 where that holds and 0.75 where not.  orc_step consumes a uniform only on an in-bounds
empty target, so this is the rule of include/tron_hip.h for any per-player rates, and the rule itself stays in the
oracle.  u is the caller's tape, or words 2 and 3 of the oracle's Philox block whose words 0 and 1 are the safe draws.
A plain module, imported by name; nothing here needs a GPU."""
import numpy as np

import oracle
import playout_support as ps

SLIDE_CLASSES = ("slide", "both_slid", "slide_to_border", "slide_to_trail", "p2_target_filled", "p1_dies_on_p2_tile")
CLASSES = SLIDE_CLASSES + ps.CLASSES
RATE_VALUES = (-1.0, 0.0, 0.03, 0.15, 0.5, 1.0, 1.5, float("nan"))


def philox_uniform(word):
    """The env's conversion of a Philox word to a slide uniform: (word >> 8) * 2^-24, a float32."""
    return (np.asarray(word, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


class SlidePlayouts(ps.Playouts):
    """n boards under the sliding rule with rates float64 [n, 2]; uniforms: float32 [K, n, 2] or None (Philox)."""

    def __init__(self, codes, rates, uniforms=None, **key):
        super().__init__(codes, **key)
        plain = self.v
        self.v = v = oracle.VecOracle(self.n, self.W, mode="ice", slide=0.5)
        v.grid[:], v.pos[:], v.done[:] = plain.grid, plain.pos, plain.done
        self.rates = np.ascontiguousarray(rates, np.float64).reshape(self.n, 2)
        self.uniforms = None if uniforms is None else np.ascontiguousarray(uniforms, np.float32)
        self.can_slide = self.rates >= 0                               # under a drawn u, which is >= 0 (NaN: False)
        self.seen = dict.fromkeys(SLIDE_CLASSES, 0)                    # steps of this call in each class, so far

    def slides(self, live):
        """bool [n, 2]: float64(u) <= rate of this step, for the live playouts (False elsewhere)."""
        if self.uniforms is not None:
            u = self.uniforms[self.t]
        else:
            u = np.ones((self.n, 2), np.float32)
            for i in np.nonzero(live & self.can_slide.any(1))[0]:      # a drawn u is >= 0: it meets no other rate
                u[i] = philox_uniform(self.philox.words(self.first_index + i, self.t)[2:])
        with np.errstate(invalid="ignore"):
            return live[:, None] & (u.astype(np.float64) <= self.rates)

    def classify(self, live, act, slides):
        """Counts this step's playouts per SLIDE_CLASSES from the position before it (orc_step decides the step itself)."""
        v, S, W = self.v, self.S, self.W
        rows = np.nonzero(live)[0]
        if not len(rows):
            return
        pos = v.pos[rows].astype(np.int64).reshape(-1, 2, 2)
        a = act[rows].astype(np.int64) & 3
        dr, dc = ps.DR[a], ps.DC[a]
        nr, nc = pos[:, :, 0] + dr, pos[:, :, 1] + dc                  # the targets
        inside = (nr >= 0) & (nc >= 0) & (nr < W) & (nc < W)
        n = (nr + 1) * S + (nc + 1)
        grid = v.grid[rows]
        take = np.arange(len(rows))[:, None]
        empty = inside & (grid[take, n] == ps.EMPTY)                   # (a head's cell is no empty cell)
        want = slides[rows]
        slid0 = empty[:, 0] & want[:, 0]
        filled = empty[:, 1] & slid0 & (n[:, 1] == n[:, 0])
        slid1 = empty[:, 1] & ~filled & want[:, 1]
        slid = np.stack([slid0, slid1], 1)
        lr, lc = nr + dr * slid, nc + dc * slid                        # where the heads land
        f = (lr + 1) * S + (lc + 1)
        landed_inside = (lr >= 0) & (lc >= 0) & (lr < W) & (lc < W)
        other_tile = np.stack([slid1 & (f[:, 0] == n[:, 1]), slid0 & (f[:, 1] == n[:, 0])], 1)
        on_trail = slid & landed_inside & ((grid[take, np.clip(f, 0, S * S - 1)] != ps.EMPTY) | other_tile)
        for name, m in (("slide", slid.any(1)), ("both_slid", slid.all(1)), ("slide_to_border", (slid & ~landed_inside).any(1)),
                        ("slide_to_trail", on_trail.any(1)), ("p2_target_filled", filled),
                        ("p1_dies_on_p2_tile", slid1 & (f[:, 0] == n[:, 1]))):
            self.seen[name] += int(m.sum())

    def step(self, row=None):
        live = self.live()
        row = np.full((self.n, 2), -1, np.int8) if row is None else np.asarray(row, np.int8)
        need = live[:, None] & (row < 0)
        act = np.where(need, self.safe_moves(need), row & 3).astype(np.int8)
        slides = self.slides(live)
        self.classify(live, act, slides)
        self.v.step(act, np.where(slides, np.float32(0.25), np.float32(0.75)), want_obs=False)
        self.t += 1

    def tally(self):
        return dict(self.seen, **super().tally())


def playout(codes, rates, actions=None, uniforms=None, k_steps=None, ks=None, **key):
    """The model of one tron_playout_slide_codes call, at several k_steps at once: {k: ((steps, winner, codes), tally)}
    for every k in `ks` (default: k_steps alone), as playout_support.playout."""
    ks = sorted(set([k_steps] if ks is None else ks))
    m = SlidePlayouts(codes, rates, uniforms, **key)
    out = {}
    for t in range(ks[-1] + 1):
        if t in ks:
            out[t] = (m.result(k0=t == 0), m.tally())
        if t < ks[-1] and m.live().any():
            m.step(None if actions is None else actions[t])
        elif t < ks[-1]:
            m.t += 1
    return out


# ---- the soups: playout_support's boards and action tapes, with rates of their own -----------------------------------
RATE_SEEDS = {4: 21, 5: 22, 10: 23, 24: 24, 32: 34}             # chosen so that widths 10 and up meet every class


def soup_rates(W, n=ps.SOUP_N, seed=None):
    """float64 [n, 2]: per board and player one of RATE_VALUES or a uniform random rate in [0, 1), independently."""
    rs = np.random.RandomState(RATE_SEEDS[W] if seed is None else seed)
    pick = rs.randint(0, len(RATE_VALUES) + 1, (n, 2))
    table = np.array(RATE_VALUES + (0.0,), np.float64)
    return np.where(pick == len(RATE_VALUES), rs.random_sample((n, 2)), table[pick])


_soup_cache = {}


def soup(W):
    """(boards, tapes, rates, {tape name: playout(...) at soup_ks(W)}) of width W under playout_support.SOUP_KEY and
    Philox uniforms, computed once per process and never changed."""
    if W not in _soup_cache:
        boards, tapes, _ = ps.soup(W)
        rates = soup_rates(W)
        model = {name: playout(boards, rates, tape, ks=ps.soup_ks(W), **ps.SOUP_KEY) for name, tape in tapes.items()}
        _soup_cache[W] = (boards, tapes, rates, model)
    return _soup_cache[W]


# ---- hand-built 4x4 boards that force the orderings of one step --------------------------------------------------------
def hand_built():
    """(boards int8 [4, 6, 6], tape int8 [1, 4, 2], rates float64 [4, 2], expected steps, winner, final codes), one step:
    0  player 1 RIGHT from (2, 1) without sliding, player 2 UP from (3, 2) sliding: its slide tile lands on player 1's new
       cell (2, 2), player 1 dies on it, player 2 wins from (1, 2); +10 shows on (2, 2)
    1  both slide: player 1's tile fills (2, 2), player 2's target, so player 2 consumes nothing and dies on it; -10 on top
    2  both slide onto the border and die there: a draw
    3  player 1 slides onto player 2's trail and dies; player 2 steps UP without sliding and wins
    (row, column) in the padded 6x6 image."""
    UP, RIGHT, LEFT = 0, 1, 3
    fresh = np.ones((6, 6), np.int8)
    fresh[0], fresh[-1], fresh[:, 0], fresh[:, -1] = -1, -1, -1, -1
    boards, final = np.stack([fresh] * 4), np.stack([fresh] * 4)
    boards[0, 2, 1], boards[0, 3, 2] = 10, -10
    final[0, 2, 1], final[0, 3, 2], final[0, 2, 2], final[0, 1, 2] = -2, -3, 10, -10
    boards[1, 2, 1], boards[1, 3, 2] = 10, -10
    final[1, 2, 1], final[1, 3, 2], final[1, 2, 2], final[1, 2, 3] = -2, -3, -10, 10
    boards[2, 2, 3], boards[2, 3, 2] = 10, -10
    final[2, 2, 3], final[2, 2, 4], final[2, 2, 5] = -2, -2, 10
    final[2, 3, 2], final[2, 3, 1], final[2, 3, 0] = -3, -3, -10
    boards[3, 2, 1], boards[3, 2, 3], boards[3, 4, 4] = 10, -3, -10
    final[3, 2, 1], final[3, 2, 2], final[3, 2, 3], final[3, 4, 4], final[3, 3, 4] = -2, -2, 10, -3, -10
    tape = np.array([[[RIGHT, UP], [RIGHT, UP], [RIGHT, LEFT], [RIGHT, UP]]], np.int8)
    rates = np.array([[-1, 1], [1, 1], [1, 1], [1, -1]], np.float64)
    return boards, tape, rates, np.ones(4, np.int32), np.array([2, 1, 0, 2], np.int8), final


# ---- the recorded sliding episodes ---------------------------------------------------------------------------------------
def recorded_rates(g):
    """float64 [episodes, 2]: what each player's uniform met in the recorded mode."""
    if str(g["mode"]) == "ice":
        return np.repeat(g["slide"].astype(np.float64)[:, None], 2, 1)
    return np.array([[oracle.get_rate(d, w) for w in ws] for d, ws in zip(g["degree"], g["weight"])], np.float64)


def suffixes(g):
    """playout_support.suffixes with the recorded uniforms and rates: (boards, tape, uniforms float32 [K, m, 2], rates
    float64 [m, 2], length, winner, final).  Past an episode's end the uniforms go on at random, like the actions."""
    boards, tape, length, winner, final = ps.suffixes(g)
    off = g["ep_off"].astype(np.int64)
    rows = np.array([t for e in range(len(off) - 1) for t in range(off[e], off[e + 1] - 1)])
    eps = np.searchsorted(off, rows, side="right") - 1
    u = np.random.RandomState(79).random_sample(tape.shape).astype(np.float32)
    for j, t in enumerate(rows):
        u[:length[j], j] = g["uniforms"][t + 1:t + 1 + length[j]]
    return boards, tape, u, recorded_rates(g)[eps], length, winner, final


def starts(g):
    """playout_support.starts with the recorded uniforms and rates."""
    boards, tape, length, winner, final = ps.starts(g)
    off = g["ep_off"].astype(np.int64)
    u = np.random.RandomState(80).random_sample(tape.shape).astype(np.float32)
    for e in range(len(length)):
        u[:length[e], e] = g["uniforms"][off[e]:off[e + 1]]
    return boards, tape, u, recorded_rates(g), length, winner, final
