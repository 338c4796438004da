"""VecTron — N independent TRON games stepped by one HIP kernel launch.

The batched counterpart of the reference's `envs = [make_game(...)] * N` list and
its `for i in range(N): envs[i].step(a1, a2)` loop (ACKTR.py:183,285-317).  All
state lives in HBM behind a `tron_handle` (include/tron_hip.h); this class only
owns the output tensors and launches kernels on torch's current stream.
"""
import ctypes as C
import numbers

import torch

from . import _native as nat

# reward tables of the three reference trainers
REWARDS = {
    "ddqn": dict(step=-1.0, win=100.0, lose=-100.0, draw=0.0, step_is_index=0),   # DDQN.py:289-305
    "dqn": dict(step=0.0, win=100.0, lose=-25.0, draw=0.0, step_is_index=1),      # DQN.py:224-241
    "acktr": dict(step=-1.0, win=10.0, lose=-10.0, draw=0.0, step_is_index=0),    # ACKTR.py:294-317 + config.py:37
}


class VecTron:
    def __init__(self, n_envs, width=10, mode=None, fair=False, seed=0x5EED, rank=0, device=None,
                 obs_format="codes", reward="ddqn", slide=None, obs_is_state=True, incremental=False):
        if not torch.cuda.is_available():
            raise nat.TronNativeError("VecTron needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.N, self.W = int(n_envs), int(width)
        self.S = self.W + 2
        self.G = self.S * self.S
        self.mode = mode
        self.seed, self.rank = seed & 0xFFFFFFFF, rank & 0xFFFFFFFF
        self.obs_format = obs_format
        self._fmt = nat.OBS[obs_format]
        self._lib = nat.lib()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_create(self.N, self.W, nat.MODE[mode], int(bool(fair)), seed & 0xFFFFFFFF,
                                            rank & 0xFFFFFFFF, C.byref(h)), "tron_create")
        self._h = h
        self.set_reward(**(REWARDS[reward] if isinstance(reward, str) else reward))
        if slide is not None:
            self.set_slide(slide)
        dev = self.device
        self.obs = self._alloc_obs(self._fmt)
        self.done = torch.zeros(self.N, dtype=torch.int8, device=dev)
        self.winner = torch.zeros(self.N, dtype=torch.int8, device=dev)
        self.reward = torch.zeros(self.N, 2, dtype=torch.float32, device=dev)
        # int8 codes + even side: let self.obs BE the env state (tron_attach_obs_state); it is then read-only for the
        # caller — clone what must outlive the next step.  (The sliding modes too: their slide tiles, which the codes show
        # as bodies, are kept in a per-env log for grid().)
        self.obs_is_state = bool(obs_is_state and self._fmt == nat.OBS_CODES_I8 and self.W % 2 == 0)
        # incremental=True (needs obs_is_state, mode None): steps write only the cells a move touches and the boards
        # that restart, instead of rewriting both planes — same observations, far less traffic
        self.incremental = bool(incremental and self.obs_is_state and mode in (None, "none"))
        if self.obs_is_state:
            with torch.cuda.device(self.device):
                nat.check(self._lib.tron_attach_obs_state(self._h, nat.ptr(self.obs), nat.stream_ptr()),
                          "tron_attach_obs_state")

    # -- plumbing ---------------------------------------------------------
    def _alloc_obs(self, fmt):
        N, S = self.N, self.S
        if fmt == nat.OBS_NONE:
            return None
        if fmt == nat.OBS_CODES_I8:
            return torch.empty(N, 2, S, S, dtype=torch.int8, device=self.device)
        ch = 3 if fmt == nat.OBS_PLANES3_F32 else 4
        return torch.empty(N, 2, ch, S, S, dtype=torch.float32, device=self.device)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tron_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dev_arg(self, t, dtype, shape):
        if t is None:
            return None
        t = torch.as_tensor(t, device=self.device).to(dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    # -- configuration ----------------------------------------------------
    def set_reward(self, step=-1.0, win=100.0, lose=-100.0, draw=0.0, step_is_index=0):
        nat.check(self._lib.tron_set_reward(self._h, step, win, lose, draw, int(step_is_index)), "tron_set_reward")

    def set_slide(self, slide):
        """Game(..., slide_pram=slide) (game.py:88); a float or a float64 [N] tensor."""
        with torch.cuda.device(self.device):
            if torch.is_tensor(slide):
                t = self._dev_arg(slide, torch.float64, (self.N,))
                nat.check(self._lib.tron_set_slide(self._h, 0.0, nat.ptr(t), nat.stream_ptr()), "tron_set_slide")
            else:
                nat.check(self._lib.tron_set_slide(self._h, float(slide), None, nat.stream_ptr()), "tron_set_slide")

    def set_weight_degree(self, weight=None, degree=None):
        """Assign Game.weight / Game.degree (game.py:83,87): int16 [N,2] / [N]."""
        w = self._dev_arg(weight, torch.int16, (self.N, 2))
        d = self._dev_arg(degree, torch.int16, (self.N,))
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_set_weight_degree(self._h, nat.ptr(w), nat.ptr(d), nat.stream_ptr()),
                      "tron_set_weight_degree")

    # -- reset / step / encode --------------------------------------------
    def reset(self, mask=None, start_pos=None, weight=None, degree=None):
        """make_game for the masked envs (all when mask is None); returns the observation."""
        m = self._dev_arg(mask, torch.int8, (self.N,))
        sp = self._dev_arg(start_pos, torch.int8, (self.N, 4))
        w = self._dev_arg(weight, torch.int16, (self.N, 2))
        d = self._dev_arg(degree, torch.int16, (self.N,))
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_reset(self._h, nat.ptr(m), nat.ptr(sp), nat.ptr(w), nat.ptr(d),
                                           nat.stream_ptr()), "tron_reset")
        return self.encode() if self._fmt != nat.OBS_NONE else None

    def step(self, actions=None, uniforms=None, autoreset=True, nonreversing=False):
        """One Game.step for every env.  actions int8 [N,2] in 0..3 (None: i.i.d. uniform
        from the env's Philox stream, or — nonreversing=True — uniform over the three headings
        that do not reverse the player's last move); uniforms f32 [N,2] for ice/temper (None: Philox).
        Returns (obs, reward, done, winner) — tensors owned by this object, overwritten by
        the next call."""
        a = self._dev_arg(actions, torch.int8, (self.N, 2))
        u = self._dev_arg(uniforms, torch.float32, (self.N, 2))
        flags = ((nat.STEP_AUTORESET if autoreset else 0) | (nat.STEP_INCREMENTAL if self.incremental else 0) |
                 (nat.STEP_NONREVERSING if nonreversing else 0))
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_step_encode(self._h, nat.ptr(a), nat.ptr(u), flags, self._fmt,
                                                 nat.ptr(self.obs), nat.ptr(self.done), nat.ptr(self.winner),
                                                 nat.ptr(self.reward), nat.stream_ptr()), "tron_step_encode")
        return self.obs, self.reward, self.done, self.winner

    def part_range(self, part, nparts):
        """(first_env, n_envs) of slice `part` of `nparts` (whole tiles of consecutive envs, split evenly)."""
        a, b = C.c_int32(), C.c_int32()
        nat.check(self._lib.tron_part_range(self._h, int(part), int(nparts), C.byref(a), C.byref(b)), "tron_part_range")
        return a.value, b.value

    def step_part(self, part, nparts, actions=None, uniforms=None, autoreset=True, nonreversing=False):
        """step() for one slice of the envs, on torch's current stream: run the slices as independent pipelines
        (one stream each) so that the policy forward of one slice overlaps the env kernel of another.  `actions`
        / `uniforms` and the returned tensors are the FULL [N, ...] buffers; only the slice's rows are read and
        written (part_range tells which)."""
        a = self._dev_arg(actions, torch.int8, (self.N, 2))
        u = self._dev_arg(uniforms, torch.float32, (self.N, 2))
        flags = (nat.STEP_AUTORESET if autoreset else 0) | (nat.STEP_NONREVERSING if nonreversing else 0)
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_step_encode_part(self._h, int(part), int(nparts), nat.ptr(a), nat.ptr(u), flags,
                                                      self._fmt, nat.ptr(self.obs), nat.ptr(self.done),
                                                      nat.ptr(self.winner), nat.ptr(self.reward), nat.stream_ptr()),
                      "tron_step_encode_part")
        return self.obs, self.reward, self.done, self.winner

    def step_fn(self, autoreset=True, nonreversing=False):
        """A zero-argument callable that launches one random-action step (Philox actions) with all
        ctypes arguments bound once — for launch loops where Python argument handling per call
        would otherwise dominate a ~25 us kernel.  Same outputs as step()."""
        fn = self._lib.tron_step_encode
        flags = ((nat.STEP_AUTORESET if autoreset else 0) | (nat.STEP_INCREMENTAL if self.incremental else 0) |
                 (nat.STEP_NONREVERSING if nonreversing else 0))
        args = (self._h, None, None, flags, self._fmt, nat.ptr(self.obs),
                nat.ptr(self.done), nat.ptr(self.winner), nat.ptr(self.reward), nat.stream_ptr())

        def launch():
            rc = fn(*args)
            if rc:
                nat.check(rc, "tron_step_encode")
        return launch

    def encode(self, obs_format=None, out=None):
        fmt = self._fmt if obs_format is None else nat.OBS[obs_format]
        if out is None:
            out = self.obs if fmt == self._fmt else self._alloc_obs(fmt)
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_encode(self._h, fmt, nat.ptr(out), nat.stream_ptr()), "tron_encode")
        return out

    def rollout_random(self, k_steps, totals=None, nonreversing=False, per_step_launches=False, two_streams=False,
                       resident=False):
        """k_steps random-action steps with autoreset (the BASELINE synthetic rollout): one persistent
        launch for up to 1 024 steps in mode None on the attached int8 codes (a longer call splits into launches of 1 024
        steps; the sliding modes: up to 64 steps each), or — per_step_launches=True — one launch per step, or — two_streams=True — one launch
        per step and per half of the envs on two streams (same results every way).  self.obs holds the observations of the
        last step once the call's work completes on the stream: a persistent launch in mode None writes them at its end, and
        only per_step_launches=True puts every step's observations into memory.  resident=True (observation-is-state
        storage): inside a persistent launch the boards stay in LDS between steps instead of being re-read from the
        observation buffer — same results, a third less HBM traffic."""
        flags = ((nat.STEP_NONREVERSING if nonreversing else 0) | (nat.ROLLOUT_PER_STEP if per_step_launches else 0) |
                 (nat.ROLLOUT_TWO_STREAMS if two_streams else 0) | (nat.ROLLOUT_RESIDENT if resident else 0))
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_rollout_random(self._h, int(k_steps), flags,
                                                    self._fmt, nat.ptr(self.obs),
                                                    nat.ptr(totals), nat.stream_ptr()), "tron_rollout_random")

    def rollout_actions(self, actions, totals=None, per_step_launches=False, records=None):
        """K steps with autoreset whose actions come from a tape: `actions` is a contiguous int8 tensor [K, N, 2] in 0..3 on
        this env's device, row k what step(actions[k]) would take (recorded games, scripted openings, a planner's candidate
        sequences, action repeat).  Same boards, state, observations and totals, bit for bit, as K calls of
        step(actions[k], autoreset=True).  Mode None on the attached int8 codes runs as one persistent launch for up to 1 024
        steps, a longer tape as launches of 1 024 (the launch of rollout_random, its action bytes copied from the tape); every other mode, side and format —
        and per_step_launches=True — is one launch per step.  self.obs holds the observations of the last step once the
        call's work completes on the stream; the tape must not be overwritten before that.
        records: None (nothing is recorded and None is returned), True, or a tuple (reward, done, winner) in the order of
        step()'s tuple.  True allocates and returns the step-major record tapes reward f32 [K, N, 2], done int8 [K, N],
        winner int8 [K, N]: row k is what step(actions[k]) returns as (reward, done, winner), for every env — when it
        finished, who won, what the step paid.  A tuple takes the caller's contiguous tensors of those dtypes and shapes
        on this device, any of them None (not recorded), and is returned as it is.  The persistent launches store the
        records as they step (tron_rollout_actions_records); the tensors hold them once the call's work completes on the
        stream."""
        _checked_tensor(actions, torch.int8, (None, self.N, 2), self.device, "rollout_actions takes an int8 tensor [K, N, 2]",
                        "rollout_actions takes int8 actions", f"expected shape (K, {self.N}, 2)", "the tape")
        K = int(actions.shape[0])
        if records is not None:
            records = self._record_tapes(records, K)
        if K == 0:
            return records
        flags = nat.ROLLOUT_PER_STEP if per_step_launches else 0
        with torch.cuda.device(self.device):
            if records is None:
                nat.check(self._lib.tron_rollout_actions(self._h, K, nat.ptr(actions), flags,
                                                         self._fmt, nat.ptr(self.obs),
                                                         nat.ptr(totals), nat.stream_ptr()), "tron_rollout_actions")
            else:
                reward, done, winner = records
                nat.check(self._lib.tron_rollout_actions_records(self._h, K, nat.ptr(actions), flags,
                                                                 self._fmt, nat.ptr(self.obs), nat.ptr(done),
                                                                 nat.ptr(winner), nat.ptr(reward),
                                                                 nat.ptr(totals), nat.stream_ptr()),
                          "tron_rollout_actions_records")
        return records

    def _record_tapes(self, records, K):
        """rollout_actions' records argument as a checked tuple (reward, done, winner)."""
        spec = (("reward", torch.float32, (K, self.N, 2)), ("done", torch.int8, (K, self.N)),
                ("winner", torch.int8, (K, self.N)))
        if records is True:
            return tuple(torch.empty(shape, dtype=dtype, device=self.device) for _, dtype, shape in spec)
        if not isinstance(records, (tuple, list)) or len(records) != 3:
            raise TypeError("records is None, True or a tuple (reward, done, winner)")
        for t, (name, dtype, shape) in zip(records, spec):
            if t is not None:
                _checked_tensor(t, dtype, shape, self.device, f"the {name} records take a {dtype} tensor {shape} or None",
                                f"the {name} records are {dtype}", f"expected {name} records of shape {shape}",
                                f"the {name} records")
        return records

    def minimax_actions(self, player, mode="voronoi", out=None, want_values=False):
        """MinimaxPlayer(2, mode).action(game.map(), player) for every env (minimax.py:284-297):
        int8 [N] actions 0..3 = UP, RIGHT, DOWN, LEFT (-1 for finished games).  With want_values
        also the root children's values int32 [N, 4] and the searched-moves bit mask int8 [N]."""
        if out is None:
            out = torch.empty(self.N, dtype=torch.int8, device=self.device)
        values = torch.empty(self.N, 4, dtype=torch.int32, device=self.device) if want_values else None
        expanded = torch.empty(self.N, dtype=torch.int8, device=self.device) if want_values else None
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_minimax_actions(self._h, int(player), 2, nat.MINIMAX[mode], nat.ptr(out),
                                                     nat.ptr(values), nat.ptr(expanded), nat.stream_ptr()),
                      "tron_minimax_actions")
        return (out, values, expanded) if want_values else out

    def playout(self, actions=None, k_steps=None, copies=1, call=0, want_codes=False, rates=None, uniforms=None,
                weights=None, judge=None):
        """playout_codes on every env's current board, `copies` times each: playout i * copies + j is env i, and the tape
        (if any) is int8 [K, N * copies, 2].  The boards are the player-1 codes — the attached buffer's plane, or a fresh
        encode("codes") — and the draws are keyed by this env's seed and rank; the env itself is left exactly as it was.
        rates=None plays mode None's rule and is for mode None only; rates=True plays the sliding rule under
        slide_rates(), a float64 [N, 2] tensor under the caller's rates (either in any mode; `uniforms`, float32
        [K, N * copies, 2], replaces the drawn slide uniforms).  weights: four ints 0..255 (HUG_WEIGHTS) weigh the drawn
        moves by their room as playout_codes does; None is the uniform draw.  Returns (steps, winner, final_codes | None)
        as playout_codes does; a finished env's row is what playout_codes makes of its image.  judge="territory": an
        unfinished playout's winner is territory_winner's verdict on its last position, as in playout_codes;
        judge="fill": fill_winner's."""
        rates = self._playout_rates(rates, "playout")
        if int(copies) < 1:
            raise ValueError("copies is at least 1")
        if rates is not None:
            rates = rates.repeat_interleave(int(copies), dim=0)
        return playout_codes(self._p1_codes().repeat_interleave(int(copies), dim=0), actions, k_steps, seed=self.seed,
                             stream_id=self.rank, call=call, want_codes=want_codes, rates=rates, uniforms=uniforms,
                             weights=weights, judge=judge)

    def territory(self, want_owner=False):
        """territory_codes on every env's current board (the player-1 codes playout takes): (counts int32 [N, 6],
        owner int8 [N, S, S] | None).  The env itself is left exactly as it was; a finished env's row is what
        territory_codes makes of its image."""
        return territory_codes(self._p1_codes(), want_owner=want_owner)

    def reach(self, want_dist=False):
        """reach_codes on every env's current board (the player-1 codes playout takes): (counts int32 [N, 8],
        dist int16 [N, 2, S, S] | None).  The env itself is left exactly as it was; a finished env's row is what
        reach_codes makes of its image."""
        return reach_codes(self._p1_codes(), want_dist=want_dist)

    def moves(self, want_actions=True):
        """moves_codes on every env's current board (the player-1 codes playout takes): (moves int32 [N, 2, 4, 3],
        actions int8 [N, 2] | None).  The env itself is left exactly as it was; a finished env's row is what moves_codes
        makes of its image."""
        return moves_codes(self._p1_codes(), want_actions=want_actions)

    def lookahead_actions(self, player, out=None):
        """The one-ply lookahead opponent, minimax_actions' and montecarlo_actions' counterpart: int8 [N], `player`'s
        (1|2) pick of moves_codes — the safe move behind which it reaches most cells first, the greater fill bound among
        equals.  One launch, no draws; no slide is looked at in any mode."""
        if int(player) not in (1, 2):
            raise ValueError("player is 1 or 2")
        actions = self.moves()[1][:, int(player) - 1]
        if out is None:
            return actions.contiguous()
        out.copy_(actions)
        return out

    def search(self, plies=2, want_actions=True):
        """search_codes on every env's current board (the player-1 codes playout takes): (values int32 [N, 2, 4],
        actions int8 [N, 2] | None).  The env itself is left exactly as it was; a finished env's row is what search_codes
        makes of its image."""
        return search_codes(self._p1_codes(), plies=plies, want_actions=want_actions)

    def search_actions(self, player, plies=2, out=None):
        """The maximin search opponent, lookahead_actions' deeper counterpart: int8 [N], `player`'s (1|2) pick of
        search_codes — the first move whose worst case over the opponent's four replies, `plies` joint moves deep with
        territory at the leaves, is greatest.  One launch, no draws; no slide is looked at in any mode."""
        if int(player) not in (1, 2):
            raise ValueError("player is 1 or 2")
        actions = self.search(plies=plies)[1][:, int(player) - 1]
        if out is None:
            return actions.contiguous()
        out.copy_(actions)
        return out

    def slide_rates(self):
        """float64 [N, 2] on the device: the rate each player's `random.random() <= rate` meets in this env's mode
        (game.py:169) — ice: the env's slide for both players; temper: get_rate(degree, weight[p]) in game.py:100-102's
        operation order, in float64; mode None: -1.0 (never).  What playout / playout_values / montecarlo_actions take as
        rates=True."""
        if self.mode in (None, "none"):
            return torch.full((self.N, 2), -1.0, dtype=torch.float64, device=self.device)
        st = self.state()
        if self.mode == "ice":
            return st["slide"].view(self.N, 1).expand(self.N, 2).contiguous()
        # every operand a device tensor: a division by a host scalar would be a multiplication by its reciprocal
        f64 = dict(dtype=torch.float64, device=self.device)
        hundred, k = torch.full((), 100.0, **f64), torch.full((), 0.6, **f64)
        a = (st["degree"].to(torch.float64) - 30.0) * k
        b = (-a) / hundred
        c = (70.0 - st["weight"].to(torch.float64)) / hundred
        return (b.view(self.N, 1) - c).contiguous()

    def _playout_rates(self, rates, what):
        """The rates argument of playout / playout_values: None (mode None only), True -> slide_rates(), or a tensor."""
        if rates is None:
            if self.mode not in (None, "none"):
                raise ValueError(f"{what} without rates plays mode None's rule; in a sliding mode pass rates=True "
                                 "(this env's slide_rates()) or a float64 [N, 2] tensor")
            return None
        if rates is True:
            return self.slide_rates()
        if not torch.is_tensor(rates):
            raise TypeError("rates is None, True or a float64 tensor [N, 2]")
        if tuple(rates.shape) != (self.N, 2):
            raise ValueError(f"expected rates of shape ({self.N}, 2), got {tuple(rates.shape)}")
        return rates

    def _p1_codes(self):
        """int8 [N, S, S] player 1's codes of the boards as they stand: the attached buffer's plane, or a fresh encode."""
        if self.obs_is_state:
            return self.obs[:, 0]
        return self.encode("codes", out=self._alloc_obs(nat.OBS_CODES_I8))[:, 0]

    def playout_values(self, k_steps, copies=1, call=0, want_actions=True, rates=None, weights=None, judge=None):
        """playout_values on every env's current board (no board is copied unless judge= is given): (counts int32 [N, 4, 4, 4], steps int32
        [N, 4, 4], actions int8 [N, 2] | None), the draws keyed by this env's seed and rank.  The env itself is left
        exactly as it was.  rates as in playout: None is mode None's rule and mode None only, True this env's
        slide_rates(), a tensor the caller's; weights and judge as in the function playout_values.  A finished env's row is
        what playout_values makes of its image."""
        rates = self._playout_rates(rates, "playout_values")
        return playout_values(self._p1_codes(), k_steps, copies, seed=self.seed, stream_id=self.rank, call=call,
                              want_actions=want_actions, rates=rates, weights=weights, judge=judge)

    def montecarlo_actions(self, player, k_steps=None, copies=4, call=0, out=None, rates=None, weights=None, judge=None):
        """The flat Monte-Carlo opponent, minimax_actions' counterpart: int8 [N], `player`'s (1|2) maximin move over the
        tallies of playout_values(k_steps, copies, call, rates=rates, weights=weights) — 16 * copies random playouts of at
        most k_steps (default W * W) steps per env.  Pass the step number as `call` so that every step draws its own
        playouts, rates=True in a sliding mode, and weights (HUG_WEIGHTS) for playouts that prefer room.  judge="territory"
        with a short k_steps judges the playouts that k_steps cuts off by territory instead of leaving them out,
        judge="fill" by the checkerboard bound on the territory each player can fill (fill_winner)."""
        if int(player) not in (1, 2):
            raise ValueError("player is 1 or 2")
        k_steps = self.W * self.W if k_steps is None else k_steps
        actions = self.playout_values(k_steps, copies, call, rates=rates, weights=weights, judge=judge)[2][:, int(player) - 1]
        if out is None:
            return actions.contiguous()
        out.copy_(actions)
        return out

    # -- read-back ---------------------------------------------------------
    def grid(self):
        """int8 [N, W+2, W+2] Tile values (map.py:9-17)."""
        out = torch.empty(self.N, self.S, self.S, dtype=torch.int8, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_get_grid(self._h, nat.ptr(out), nat.stream_ptr()), "tron_get_grid")
        return out

    def state(self):
        dev, N = self.device, self.N
        out = dict(pos=torch.empty(N, 4, dtype=torch.int8, device=dev),
                   alive=torch.empty(N, 2, dtype=torch.int8, device=dev),
                   dir=torch.empty(N, 2, dtype=torch.int8, device=dev),
                   done=torch.empty(N, dtype=torch.int8, device=dev),
                   winner=torch.empty(N, dtype=torch.int8, device=dev),
                   weight=torch.empty(N, 2, dtype=torch.int16, device=dev),
                   degree=torch.empty(N, dtype=torch.int16, device=dev),
                   slide=torch.empty(N, dtype=torch.float64, device=dev),
                   counters=torch.empty(N, 3, dtype=torch.int32, device=dev))
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_get_state(self._h, *[nat.ptr(out[k]) for k in
                                                          ("pos", "alive", "dir", "done", "winner", "weight",
                                                           "degree", "slide", "counters")],
                                               nat.stream_ptr()), "tron_get_state")
        return out


def encode_codes(tiles, player):
    """Map.state_for_player(player) on a stack of raw tile images (map.py:67-84)."""
    t = tiles.contiguous()
    out = torch.empty_like(t)
    n = t.shape[0] if t.dim() > 2 else 1
    nat.check(nat.lib().tron_encode_codes(nat.ptr(t), n, t.numel() // n, int(player), nat.ptr(out),
                                          nat.stream_ptr()), "tron_encode_codes")
    return out


def minimax_codes(codes, draws=None, mode="voronoi", depth=2):
    """The reference's MinimaxPlayer(depth, mode) search (minimax.py:216-297) on a stack of
    observation-code images int8 [n, S, S] of the player to move.  Returns (actions int8 [n] in
    0..3 = UP, RIGHT, DOWN, LEFT, root values int32 [n, 4], searched-moves bit mask int8 [n]).
    draws: uint32-valued int64/int32 tensor [n] for random.choice / randint (None = zeros)."""
    c = codes.contiguous()
    n, side = c.shape[0], c.shape[-1]
    act = torch.empty(n, dtype=torch.int8, device=c.device)
    values = torch.empty(n, 4, dtype=torch.int32, device=c.device)
    expanded = torch.empty(n, dtype=torch.int8, device=c.device)
    d = None
    if draws is not None:
        d = draws.to(torch.int64) & 0xFFFFFFFF
        d = torch.where(d >= 2 ** 31, d - 2 ** 32, d).to(torch.int32).contiguous()      # same 32 bits
    with torch.cuda.device(c.device):
        nat.check(nat.lib().tron_minimax_codes(nat.ptr(c), n, side, int(depth), nat.MINIMAX[mode], nat.ptr(d),
                                               nat.ptr(act), nat.ptr(values), nat.ptr(expanded), nat.stream_ptr()),
                  "tron_minimax_codes")
    return act, values, expanded


def _fits(t, shape):
    """Whether tensor t has the shape `shape`, in which None stands for any size."""
    return t.dim() == len(shape) and all(want is None or want == got for want, got in zip(shape, t.shape))


def _checked_tensor(t, dtype, shape, device, takes, is_dtype, of_shape, name):
    """The check of a tensor argument: a tensor, of `dtype`, of `shape` (None: any size), on `device`, contiguous — in
    that order, each fault with its own exception.  The last four arguments are the argument's name as its messages
    spell it: the whole message for something that is no tensor, the openings of the dtype and the shape message (", got
    ..." follows), and the subject of "... must be on ..." and "... must be contiguous"."""
    if not torch.is_tensor(t):
        raise TypeError(takes)
    if t.dtype != dtype:
        raise TypeError(f"{is_dtype}, got {t.dtype}")
    if not _fits(t, shape):
        raise ValueError(f"{of_shape}, got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{name} must be on {device}, got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _slide_rates(rates, n, device, what):
    """The checked rates argument of playout_codes / playout_values: float64 [n, 2], contiguous, on the boards' device."""
    return _checked_tensor(rates, torch.float64, (n, 2), device, f"{what}: rates is None or a float64 tensor [n, 2]",
                           f"{what}: rates are float64", f"{what}: expected rates of shape ({n}, 2)", f"{what}: rates")


def _boards(codes, what):
    """The boards argument of `what` as (contiguous int8 [n, S, S], n, S)."""
    c = codes.contiguous()
    if c.dtype != torch.int8 or c.dim() != 3 or c.shape[1] != c.shape[2]:
        raise ValueError(f"{what} takes int8 boards [n, S, S], got {c.dtype} {tuple(c.shape)}")
    return c, int(c.shape[0]), int(c.shape[-1])


def _key(seed, stream_id, call):
    """(seed, stream_id, call) as the entries take them: 32, 32 and 64 bits."""
    return seed & 0xFFFFFFFF, stream_id & 0xFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF


def _playout_entry(kind, head, sliding, packed, key, outs):
    """Calls the "codes" or "values" entry that the arguments choose: tron_playout_weighted_<kind> under weights (which
    takes the sliding rule's tensors too, None for mode None's rule), else tron_playout_<kind> where rates, the first of
    `sliding`, is None, else tron_playout_slide_<kind>.  head: the arguments before them, outs: the output tensors."""
    if packed is not None:
        name, chosen = f"tron_playout_weighted_{kind}", (*map(nat.ptr, sliding), packed)
    elif sliding[0] is None:
        name, chosen = f"tron_playout_{kind}", ()
    else:
        name, chosen = f"tron_playout_slide_{kind}", tuple(map(nat.ptr, sliding))
    nat.check(getattr(nat.lib(), name)(*head, *chosen, *key, *map(nat.ptr, outs), nat.stream_ptr()), name)


HUG_WEIGHTS = (0, 4, 2, 1)                                              # measured: profiles/r27_playout_policy_match.txt


def _packed_weights(weights, what):
    """The checked weights argument of playout_codes / playout_values as the entries take it: byte k is w[k]."""
    try:
        w = list(weights)
    except TypeError:
        raise TypeError(f"{what}: weights is None or a sequence of four ints 0..255") from None
    if len(w) != 4:
        raise ValueError(f"{what}: weights are four, one per room 0..3, got {len(w)}")
    if not all(isinstance(x, numbers.Integral) and not isinstance(x, bool) for x in w):
        raise TypeError(f"{what}: weights are ints, got {[type(x).__name__ for x in w]}")
    if not all(0 <= x <= 255 for x in w):
        raise ValueError(f"{what}: weights are 0..255, got {[int(x) for x in w]}")
    return sum(int(x) << (8 * k) for k, x in enumerate(w))


def playout_codes(codes, actions=None, k_steps=None, seed=0x5EED, stream_id=0, call=0, want_codes=False, rates=None,
                  uniforms=None, weights=None, judge=None):
    """Plays a stack of observation-code boards int8 [n, S, S] (player 1's view: encode_codes(.., 1), a VecTron's
    obs[:, 0]) forward up to k_steps steps of mode None's Game.step, without restart (tron_playout_codes).  Returns
    (steps int32 [n], winner int8 [n], final_codes int8 [n, S, S] or None): steps played, 0 draw / 1 / 2 / -1 not
    finished / -2 rejected (not exactly one +10 and one -10 inside the border), and — want_codes=True — player 1's
    observation of the last position reached.  actions: int8 tape [K, n, 2], step-major; a byte 0..127 is an action (its
    low two bits), a negative byte draws a safe move for that player in that step; None draws every move.  k_steps
    defaults to the tape's length.  The draws are Philox keyed by (seed, stream_id) at counter (playout, step, call):
    pass another `call` for another set of playouts of the same boards; a fork is a repeat_interleave of the codes.
    rates: float64 [n, 2] on the boards' device plays the sliding rule of "ice" / "temper" instead
    (tron_playout_slide_codes): player p of board i slides when (double)u <= rates[i, p], u from words 2 and 3 of the
    step's Philox block, or from `uniforms`, a float32 tape [K, n, 2]; a slide tile shows as its owner's body.
    weights: four ints 0..255 weigh every drawn move by its room under either rule (tron_playout_weighted_codes):
    weights[k] is the weight of a safe move whose target has k EMPTY cells among its three neighbours other than the
    mover's head, and the move is the first safe one whose running sum of weights exceeds mulhi(u, sum) at the word u the
    uniform draw uses; safe moves that all weigh 0 are drawn uniformly.  Four equal weights are the uniform draw bit
    for bit; HUG_WEIGHTS is a preset that prefers tight cells.  None calls the entries without weights.
    judge: None, or "territory": a playout that comes back unfinished (winner -1) has its last position judged by
    territory_winner(territory_codes(final)), and the returned winner carries that verdict (1, 2, or 0 for equal
    territory) in the place of -1; steps and codes are as without it.  "fill" does the same with
    fill_winner(reach_codes(final)), the verdict of the checkerboard bound.  The last positions are computed whether or
    not want_codes asks for them."""
    _checked_judge(judge, "playout_codes")
    c, n, side = _boards(codes, "playout_codes")
    packed = None if weights is None else _packed_weights(weights, "playout_codes")
    a = None
    if actions is not None:                                            # one message for dtype and shape; any strides
        if actions.dtype != torch.int8 or not _fits(actions, (None, n, 2)):
            raise ValueError(f"expected an int8 tape of shape (K, {n}, 2), got {actions.dtype} {tuple(actions.shape)}")
        a = actions.contiguous()
        if k_steps is None:
            k_steps = int(a.shape[0])
        elif int(k_steps) > int(a.shape[0]):
            raise ValueError(f"k_steps {k_steps} is more than the tape's {int(a.shape[0])} rows")
    if uniforms is not None:
        if rates is None:
            raise ValueError("uniforms belong to the sliding rule: pass rates with them")
        _checked_tensor(uniforms, torch.float32, (None, n, 2), c.device, "uniforms is None or a float32 tensor [K, n, 2]",
                        "the uniforms are float32", f"expected a float32 uniforms tape of shape (K, {n}, 2)", "the uniforms")
        if k_steps is None:
            k_steps = int(uniforms.shape[0])
        elif int(k_steps) > int(uniforms.shape[0]):
            raise ValueError(f"k_steps {k_steps} is more than the uniforms tape's {int(uniforms.shape[0])} rows")
    if k_steps is None:
        raise ValueError("playout_codes needs k_steps when there is no tape")
    if rates is not None:
        rates = _slide_rates(rates, n, c.device, "playout_codes")
    cp, ap = nat.ptr(c), nat.ptr(a)                                   # host tensors are refused here
    if a is not None and a.device != c.device:
        raise ValueError(f"the tape must be on {c.device}, got {a.device}")
    steps = torch.empty(n, dtype=torch.int32, device=c.device)
    winner = torch.empty(n, dtype=torch.int8, device=c.device)
    final = torch.empty_like(c) if want_codes or judge is not None else None
    with torch.cuda.device(c.device):
        _playout_entry("codes", (cp, n, side, int(k_steps), ap), (rates, uniforms), packed, _key(seed, stream_id, call),
                       (steps, winner, final))
    if judge is not None:
        winner = torch.where(winner == -1, _VERDICTS[judge](final), winner)
    return steps, winner, (final if want_codes else None)


# judge= of the playout calls: the verdict int8 [n] on a stack of last positions
_VERDICTS = {"territory": lambda final: territory_winner(territory_codes(final)[0]),
             "fill": lambda final: fill_winner(reach_codes(final)[0])}


def _checked_judge(judge, what):
    if not (judge is None or (isinstance(judge, str) and judge in _VERDICTS)):
        raise ValueError(f'{what}: judge is None or "territory", got {judge!r}')      # or "fill": the older text is kept


def territory_codes(codes, want_owner=False):
    """Who reaches which cell first on a stack of observation-code boards int8 [n, S, S] (tron_territory_codes; the boards
    playout_codes takes).  Returns (counts int32 [n, 6], owner int8 [n, S, S] or None).  Over a board's open cells — byte
    1, strictly inside the border; the heads' cells and the border ring are closed — and the breadth-first distances d1,
    d2 from the +10 and the -10 head: counts = (first1: d1 < d2, first2: d2 < d1, tied: d1 = d2 finite, neither: both
    infinite, reach1: d1 finite, reach2: d2 finite).  reach1 + reach2 - (first1 + first2 + tied) is 0 exactly when the
    players are cut off from each other.  owner: 1, 2, 3 on first1, first2 and tied cells, 0 elsewhere.  A rejected board
    (not exactly one +10 and one -10 inside the border) gets six -1 and an owner plane of zeros."""
    c, n, side = _boards(codes, "territory_codes")
    cp = nat.ptr(c)                                                    # a host tensor is refused here
    counts = torch.empty(n, 6, dtype=torch.int32, device=c.device)
    owner = torch.empty_like(c) if want_owner else None
    with torch.cuda.device(c.device):
        nat.check(nat.lib().tron_territory_codes(cp, n, side, nat.ptr(counts), nat.ptr(owner), nat.stream_ptr()),
                  "tron_territory_codes")
    return counts, owner


def territory_winner(counts):
    """The verdict of territory_codes' counts [n, 6] as playout_codes reports winners, int8 [n]: -2 for a rejected row, else
    1 / 2 for the player that reaches more cells first, 0 for equal territory."""
    first1, first2 = counts[:, 0], counts[:, 1]
    verdict = (first1 < first2).to(torch.int8) * 2 + (first1 > first2).to(torch.int8)
    return torch.where(first1 < 0, torch.full_like(verdict, -2), verdict)


def reach_codes(codes, want_dist=False):
    """How far each player is from every cell of a stack of observation-code boards int8 [n, S, S] (tron_reach_codes; the
    boards, open cells and distances d1, d2 of territory_codes).  Returns (counts int32 [n, 8], dist int16 [n, 2, S, S] or
    None).  dist[i, p] holds d_(p+1) where finite, 0 on that head's own cell, -1 elsewhere.  counts = (opp1, same1, opp2,
    same2, fill1, fill2, depth1, depth2): territory_codes' first1 / first2 cells split by checkerboard colour (r + c) & 1
    into those of the head's own colour (same) and the others (opp); fill_p = 2 * same_p + 1 if opp_p > same_p else
    2 * opp_p, the longest colour-alternating walk from beside the head those cells allow, an upper bound on the moves
    player p can make in the cells it reaches first; depth_p the largest finite d_p.  A rejected board (not exactly one
    +10 and one -10 inside the border) gets eight -1 and planes of -1."""
    c, n, side = _boards(codes, "reach_codes")
    cp = nat.ptr(c)                                                    # a host tensor is refused here
    counts = torch.empty(n, 8, dtype=torch.int32, device=c.device)
    dist = torch.empty(n, 2, side, side, dtype=torch.int16, device=c.device) if want_dist else None
    with torch.cuda.device(c.device):
        nat.check(nat.lib().tron_reach_codes(cp, n, side, nat.ptr(counts), nat.ptr(dist), nat.stream_ptr()), "tron_reach_codes")
    return counts, dist


def fill_winner(counts):
    """The verdict of reach_codes' counts [n, 8] as playout_codes reports winners, int8 [n]: -2 for a rejected row, else
    1 / 2 for the player whose fill bound is greater, 0 for equal bounds."""
    fill1, fill2 = counts[:, 4], counts[:, 5]
    verdict = (fill1 < fill2).to(torch.int8) * 2 + (fill1 > fill2).to(torch.int8)
    return torch.where(fill1 < 0, torch.full_like(verdict, -2), verdict)


def moves_codes(codes, want_actions=True):
    """What each move of a stack of observation-code boards int8 [n, S, S] leads into (tron_moves_codes; the boards, open
    cells and distances of territory_codes).  Returns (moves int32 [n, 2, 4, 3], actions int8 [n, 2] or None).
    moves[i, p, a] = (room, fill, first) of player p's (0: the +10 head) move in direction a = UP, RIGHT, DOWN, LEFT, three
    -1 where the target is no open cell: room the open cells the flood from the target reaches, the target among them;
    fill the checkerboard bound on the moves the player can still make, this one included (reach_codes' bound started on
    the target); first the reached cells the player stands on before the opponent can, the step counted (1 + e < d_q).
    actions[i, p] = the first direction of the greatest (first, fill), 0 when no move is safe.  A rejected board (not
    exactly one +10 and one -10 inside the border) gets 24 times -1 and actions of -1."""
    c, n, side = _boards(codes, "moves_codes")
    cp = nat.ptr(c)                                                    # a host tensor is refused here
    moves = torch.empty(n, 2, 4, 3, dtype=torch.int32, device=c.device)
    actions = torch.empty(n, 2, dtype=torch.int8, device=c.device) if want_actions else None
    with torch.cuda.device(c.device):
        nat.check(nat.lib().tron_moves_codes(cp, n, side, nat.ptr(moves), nat.ptr(actions), nat.stream_ptr()), "tron_moves_codes")
    return moves, actions


def safe_moves(moves):
    """moves_codes' moves [n, 2, 4, 3] as safe-move masks, bool [n, 2, 4]: room >= 0."""
    return moves[..., 0] >= 0


SEARCH_REJECTED = -2 ** 31                                             # search_codes' eight values of a rejected board


def search_codes(codes, plies=2, want_actions=True):
    """Exact maximin move values of a stack of observation-code boards int8 [n, S, S], `plies` = 1, 2 or 3 joint moves deep
    (tron_search_codes; the boards and open cells of territory_codes).  Returns (values int32 [n, 2, 4], actions int8
    [n, 2] or None).  T_p(a) is the cell beside head p (0: the +10 head) in direction a = UP, RIGHT, DOWN, LEFT, and the
    move is safe when that cell is open.  A joint move (a for player 1, b for player 2) follows mode None's step rule:
    both unsafe, or both safe onto the same cell, is a draw; exactly one unsafe, the other player wins; otherwise the
    child position has both targets closed and the heads on them, the old head cells staying closed.  At a node reached
    after k joint moves with r plies left, V_p = first_p - first_q of territory_codes when r = 0; else V_p = max over a
    of U_p(a), U_p(a) = min over all four b of W_p(a, b), W_p = 0 on a draw, +(2048 - k) if p wins the joint move,
    -(2048 - k) if p loses it, V_p(child, r - 1) otherwise.  All 16 joint moves are judged by the rule; V_1 and V_2 are
    separate maximins over the same leaves.  values[i, p, a] = the root's U_p(a); actions[i, p] = the first direction of
    the greatest U_p, always 0..3 on a playable board.  A rejected board (not exactly one +10 and one -10 inside the
    border) gets eight SEARCH_REJECTED and actions of -1."""
    c, n, side = _boards(codes, "search_codes")
    cp = nat.ptr(c)                                                    # a host tensor is refused here
    values = torch.empty(n, 2, 4, dtype=torch.int32, device=c.device)
    actions = torch.empty(n, 2, dtype=torch.int8, device=c.device) if want_actions else None
    with torch.cuda.device(c.device):
        nat.check(nat.lib().tron_search_codes(cp, n, side, int(plies), nat.ptr(values), nat.ptr(actions), nat.stream_ptr()),
                  "tron_search_codes")
    return values, actions


def playout_values(codes, k_steps, copies=1, seed=0x5EED, stream_id=0, call=0, want_actions=True, rates=None, weights=None,
                   judge=None):
    """Monte-Carlo move values of a stack of observation-code boards int8 [n, S, S] (tron_playout_values): every board is
    played 16 * copies times, `copies` playouts behind each joint first move (a1, a2), every later move a safe draw.
    Playout (i, a1, a2, j) is what playout_codes does at launch index q = ((i * 16 + a1 * 4 + a2) * copies + j) with board
    i there and (a1, a2) in the tape's first row, under the same (seed, stream_id, call); no copied board and no tape is
    made.  Returns (counts int32 [n, 4, 4, 4], steps int32 [n, 4, 4], actions int8 [n, 2] or None): counts[i, a1, a2] =
    how many of those playouts ended as a draw, a win of player 1, a win of player 2, or not within k_steps (all zero for
    a rejected board); steps = the sum of their lengths; actions[i, p] = player p + 1's maximin move on wins of 1 minus
    wins of 2 (the first of equal moves in UP, RIGHT, DOWN, LEFT order; -1 for a rejected board).
    rates: float64 [n, 2] on the boards' device plays the sliding rule (tron_playout_slide_values): board i's row serves
    all its playouts, which are playout_codes(rates=...)'s at the same index, with drawn uniforms.
    weights: four ints 0..255 as in playout_codes (tron_playout_weighted_values): every move behind the first is
    playout_codes(weights=...)'s at the same index, under either rule.
    judge: None, "territory" or "fill": the playouts that k_steps cuts off are judged (playout_codes(judge=...)) and
    tallied under that verdict, so counts[..., 3] is 0.  This is the composition the definition above names, actually
    made: the boards copied 16 * copies times, the tape, playout_codes at the same key (playout q has the Philox index q
    it has without judge, so where no playout is left unfinished the counts are the same), the judge's call on the last
    positions, the tallies summed on the device and tron_values_pick.  Memory: two code planes (the copy and the last
    position, 2 * S * S bytes) and 2 * k_steps tape bytes per playout, n * 16 * copies playouts."""
    _checked_judge(judge, "playout_values")
    c, n, side = _boards(codes, "playout_values")
    packed = None if weights is None else _packed_weights(weights, "playout_values")
    k_steps, copies = int(k_steps), int(copies)
    if k_steps < 0:
        raise ValueError("k_steps is at least 0")
    if copies < 1:
        raise ValueError("copies is at least 1")
    if n * 16 * copies >= 2 ** 31:
        raise ValueError(f"{n} boards x 16 moves x {copies} copies do not fit the 32-bit playout index")
    if copies * k_steps >= 2 ** 31:
        raise ValueError(f"{copies} copies x {k_steps} steps do not fit a 32-bit sum of steps")
    if rates is not None:
        rates = _slide_rates(rates, n, c.device, "playout_values")
    cp = nat.ptr(c)                                                    # a host tensor is refused here
    if judge is not None:
        return _judged_values(c, k_steps, copies, seed, stream_id, call, want_actions, rates, weights, judge)
    counts = torch.empty(n, 4, 4, 4, dtype=torch.int32, device=c.device)
    steps = torch.empty(n, 4, 4, dtype=torch.int32, device=c.device)
    actions = torch.empty(n, 2, dtype=torch.int8, device=c.device) if want_actions else None
    with torch.cuda.device(c.device):
        _playout_entry("values", (cp, n, side, k_steps, copies), (rates,), packed, _key(seed, stream_id, call),
                       (counts, steps, actions))
    return counts, steps, actions


def _judged_values(c, k_steps, copies, seed, stream_id, call, want_actions, rates, weights, judge):
    """playout_values(judge=...) on checked arguments: the fan-out, playout_codes, the tallies, the pick."""
    n, per = int(c.shape[0]), 16 * copies
    tape = torch.full((k_steps, n * per, 2), -1, dtype=torch.int8, device=c.device)
    if k_steps:
        move = (torch.arange(n * per, device=c.device) // copies) % 16
        tape[0, :, 0], tape[0, :, 1] = (move >> 2).to(torch.int8), (move & 3).to(torch.int8)
    if rates is not None:
        rates = rates.repeat_interleave(per, dim=0)
    steps, winner, _ = playout_codes(c.repeat_interleave(per, dim=0), tape, k_steps, seed=seed, stream_id=stream_id, call=call,
                                     rates=rates, weights=weights, judge=judge)
    winner = winner.view(n, 4, 4, copies)
    counts = torch.stack([(winner == w).sum(-1, dtype=torch.int32) for w in (0, 1, 2, -1)], -1).contiguous()
    total = steps.view(n, 4, 4, copies).sum(-1, dtype=torch.int32)
    actions = None
    if want_actions:
        actions = torch.empty(n, 2, dtype=torch.int8, device=c.device)
        with torch.cuda.device(c.device):
            nat.check(nat.lib().tron_values_pick(nat.ptr(counts), n, nat.ptr(actions), nat.stream_ptr()), "tron_values_pick")
    return counts, total, actions


def pop_up_planes(codes):
    """util.pop_up on a stack of code planes [n, S, S] -> f32 [n, 3, S, S] (util.py:11-37)."""
    c = codes.contiguous()
    n, cells = c.shape[0], c[0].numel()
    out = torch.empty((n, 3) + tuple(c.shape[1:]), dtype=torch.float32, device=c.device)
    nat.check(nat.lib().tron_pop_up(nat.ptr(c), n, cells, nat.ptr(out), nat.stream_ptr()), "tron_pop_up")
    return out


class DeviceReplay:
    """HBM ring of transitions — DDQN.ReplayBuffer (DDQN.py:167-203) without the host."""

    def __init__(self, capacity, cells, seed=0x5EED, rank=0, device=None):
        if not torch.cuda.is_available():
            raise nat.TronNativeError("DeviceReplay needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.capacity, self.cells = int(capacity), int(cells)
        self._lib = nat.lib()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_replay_create(self.capacity, self.cells, seed & 0xFFFFFFFF, rank & 0xFFFFFFFF,
                                                   C.byref(h)), "tron_replay_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tron_replay_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        size = C.c_int64()
        nat.check(self._lib.tron_replay_size(self._h, C.byref(size), None))
        return size.value

    def add(self, state, action, reward, next_state, done):
        """Batched ReplayBuffer.add: state/next_state int8 [n, cells...] codes, action int8 [n],
        reward f32 [n], done int8 [n]."""
        n = next_state.shape[0]
        # every converted tensor stays bound to a local until the call returns: a temporary freed
        # right after nat.ptr() could be handed to the next conversion by the caching allocator
        # before the push kernel has read it
        s2 = next_state.reshape(n, -1).to(torch.int8).contiguous()
        s = s2 if state is None else state.reshape(n, -1).to(torch.int8).contiguous()     # None: add_states() wrote them
        a = action.reshape(n).to(torch.int8).contiguous()
        r = reward.reshape(n).to(torch.float32).contiguous()
        d = done.reshape(n).to(torch.int8).contiguous()
        if s.shape[1] != self.cells or s2.shape[1] != self.cells:
            raise ValueError(f"states must have {self.cells} cells per row, got {s.shape[1]} / {s2.shape[1]}")
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_replay_push(self._h, n, None if state is None else nat.ptr(s), nat.ptr(a), nat.ptr(r),
                                                 nat.ptr(s2), nat.ptr(d), nat.stream_ptr()), "tron_replay_push")
        del s, s2, a, r, d

    def add_states(self, state):
        """The `state` rows of the next add(), written ahead of it (tron_replay_push_states): call before the env step
        overwrites an observation buffer that is the env state, then add(None, action, reward, next_state, done)."""
        n = state.shape[0]
        s = state.reshape(n, -1)
        if s.dtype != torch.int8 or not s.is_contiguous() or s.shape[1] != self.cells:
            raise ValueError(f"add_states takes contiguous int8 rows of {self.cells} cells")
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_replay_push_states(self._h, n, nat.ptr(s), nat.stream_ptr()), "tron_replay_push_states")

    def sample(self, batch, channels=3, plane4=0.0, side=None):
        """ReplayBuffer.sample(): (states, actions, rewards, next_states, dones) on the device,
        states f32 [batch, channels, S, S], actions i64 [batch,1], rewards/dones f32 [batch,1]."""
        dev = self.device
        S = side if side is not None else int(round(self.cells ** 0.5))
        st = torch.empty(batch, channels, S, S, dtype=torch.float32, device=dev)
        s2 = torch.empty_like(st)
        a = torch.empty(batch, 1, dtype=torch.int64, device=dev)
        r = torch.empty(batch, 1, dtype=torch.float32, device=dev)
        d = torch.empty(batch, 1, dtype=torch.float32, device=dev)
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_replay_sample(self._h, batch, channels, float(plane4), nat.ptr(st), nat.ptr(a),
                                                   nat.ptr(r), nat.ptr(s2), nat.ptr(d), nat.stream_ptr()),
                      "tron_replay_sample")
        return st, a, r, s2, d

    def sample_codes(self, batch, side=None):
        """The same draw with the states left as int8 observation codes [batch, S, S] (tron_replay_sample_codes): what
        the learner's conv1 and the weight-stationary target forwards read — a twelfth of the bytes of the f32 planes."""
        dev = self.device
        S = side if side is not None else int(round(self.cells ** 0.5))
        st = torch.empty(batch, S, S, dtype=torch.int8, device=dev)
        s2 = torch.empty_like(st)
        a = torch.empty(batch, 1, dtype=torch.int64, device=dev)
        r = torch.empty(batch, 1, dtype=torch.float32, device=dev)
        d = torch.empty(batch, 1, dtype=torch.float32, device=dev)
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_replay_sample_codes(self._h, batch, nat.ptr(st), nat.ptr(a), nat.ptr(r), nat.ptr(s2),
                                                         nat.ptr(d), nat.stream_ptr()), "tron_replay_sample_codes")
        return st, a, r, s2, d

    def cursor(self):
        """(write head, filled slots, sample() calls so far): tron_replay_get_cursor."""
        head, size, calls = C.c_int64(), C.c_int64(), C.c_uint32()
        nat.check(self._lib.tron_replay_get_cursor(self._h, C.byref(head), C.byref(size), C.byref(calls)), "tron_replay_get_cursor")
        return head.value, size.value, calls.value

    def state_dict(self, contents=True):
        """The ring for a checkpoint ("replay head"): the cursor always; with contents=True also the filled
        slots of all five arrays as HOST tensors (2 * cells + 6 bytes per slot: 1.35 GB for 1 M slots at 24x24 boards) —
        slots [0, size), in ring order, so that load_state_dict puts every transition back where it was."""
        head, size, calls = self.cursor()
        out = {"capacity": self.capacity, "cells": self.cells, "head": head, "size": size, "sample_calls": calls}
        if contents and size > 0:
            dev = self.device
            s = torch.empty(size, self.cells, dtype=torch.int8, device=dev)
            s2 = torch.empty_like(s)
            a = torch.empty(size, dtype=torch.int8, device=dev)
            r = torch.empty(size, dtype=torch.float32, device=dev)
            d = torch.empty(size, dtype=torch.int8, device=dev)
            with torch.cuda.device(dev):
                nat.check(self._lib.tron_replay_export(self._h, 0, size, nat.ptr(s), nat.ptr(s2), nat.ptr(a), nat.ptr(r), nat.ptr(d),
                                                       nat.stream_ptr()), "tron_replay_export")
            out.update(states=s.cpu(), next_states=s2.cpu(), actions=a.cpu(), rewards=r.cpu(), dones=d.cpu())
        return out

    def load_state_dict(self, sd):
        """Inverse of state_dict(): the cursor, and the contents when the checkpoint holds them (a cursor-only checkpoint
        into a ring that has fewer slots filled than it claims is refused: sampling would read slots nobody wrote)."""
        if int(sd["capacity"]) != self.capacity or int(sd["cells"]) != self.cells:
            raise ValueError(f"checkpointed ring is {sd['capacity']} x {sd['cells']}, this one {self.capacity} x {self.cells}")
        size = int(sd["size"])
        if "states" in sd:
            dev = self.device
            t = [sd[k].to(dev).contiguous() for k in ("states", "next_states", "actions", "rewards", "dones")]
            if t[0].shape != (size, self.cells) or t[0].dtype != torch.int8 or t[3].dtype != torch.float32:
                raise ValueError("checkpointed ring contents do not match its cursor")
            with torch.cuda.device(dev):
                nat.check(self._lib.tron_replay_import(self._h, 0, size, *[nat.ptr(x) for x in t], nat.stream_ptr()), "tron_replay_import")
                torch.cuda.current_stream().synchronize()              # (t is freed on return)
        elif size > len(self):
            raise ValueError("cursor-only replay checkpoint: the ring holds fewer transitions than the cursor says")
        nat.check(self._lib.tron_replay_set_cursor(self._h, int(sd["head"]), size, int(sd["sample_calls"])), "tron_replay_set_cursor")

    def last_indices(self, batch):
        out = torch.empty(batch, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            nat.check(self._lib.tron_replay_indices(self._h, batch, nat.ptr(out), nat.stream_ptr()))
        return out
