#!/usr/bin/env python3
"""Per-step phase times of k_obs_roll (roll_resident) from a -DTRON_STAMPS diagnostic build (development tool).
Build:  csrc/build.sh -DTRON_STAMPS  (or one such libtron_hip.so named by TRON_HIP_LIB), then run this on the GPU.
The build stamps every step of a launch and the launch itself: [workgroups][2 waves][TRON_ROLLOUT_CHUNK + 1][4 slots] of
s_memrealtime ticks (100 MHz).  Slots of a step: 0 step start, 1 move done, 2 a restarted env's state words, board and next
starts done (before the restart was one region: its board rebuilt, the next game drawn in 2->3; before the planes were
written once per launch: the step's plane stores issued), 3 records done (before the helper waves: + the next step's Philox
block).  Compare 1->3 across libraries of both kinds.  Slots of the last block: 0 kernel entry, 1 step loop left, 2 the
launch's plane stores issued, 3 kernel end.
The workgroup is game waves (the low half of its wave indices) and as many helper waves; these rows are the game waves': waves 0 and 1
of a four-wave-shape workgroup, wave 0 of a one-wave-shape one (its wave 1 is the helper).  The one barrier per block of
--block steps (ROLL_R) sits between slot 3 of the block's last step and slot 0 of the next one: the gap 3 -> 0' is printed for
those steps and for the others; a library from before the helper waves shows the same gap in both rows.
--old-layout reads a library from before the launch block existed ([TRON_ROLLOUT_CHUNK][4] per wave).
Helper rows (a library whose helpers stamp; none are printed for an older one).  Behind the game waves' region, at ceil(N / 64)
* 2 * (TRON_ROLLOUT_CHUNK + 1) * 4, the helper of each stamped game wave has 4 + 2 * TRON_ROLLOUT_CHUNK / ROLL_R slots: 0
kernel entry, 1 prologue draws done, 2 arrival at P, 3 departure from P, 2 + 2 b / 3 + 2 b arrival at / departure from the
barrier B_b in front of block b; the last slot but one is the end of the hand-off pass (the helper's last block: the next
launch's first starts and action bytes, stored for it), zero in a library from before it; the last slot is the game wave's
arrival at P.  Run once as it is (the handed entry: every launch after the first takes what the one before it handed over)
and once with TRON_ROLL_NO_HANDOFF=1 (the draw entry); the header line says which, and the rows "P: helper's arrival -
game's", "helper: block 0's work" (its top-up) and "B_1: helper's arrival - game's" are the ones the two entries differ in.  A game wave arrives at B_b with slot 3 of
step b R - 1 and leaves it with slot 0 of step b R.  Printed per role: the work of a block (release of B_b -> arrival at
B_(b+1)), the wait at the barriers, and per barrier which role of a pair arrives last and by how much (helper - game).
--steps K: the launches are K steps long (default 64; 320 is the benchmark's call as one launch).  The regions are not
longer for it: a build stamps the first TRON_ROLLOUT_CHUNK = 64 steps and the barriers of the first 8 blocks, and the
launch-level slots (kernel entry, loop left, stores issued, kernel end; the hand-off pass's end) are the whole launch's.  The
per-step rows are then those of the first 64 steps; "step loop" and "first kernel entry -> last kernel end" are the K steps'.
usage: roll_stamps.py [--envs N] [--launches L] [--block R] [--steps K] [--old-layout]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "deep-q-learning_tron_amd")]


def main():
    import torch
    import tron.vec as tv                                       # the repository's package (ROOT/deep-q-learning_tron_amd/tron)

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--old-layout", action="store_true")
    a = ap.parse_args()
    N, W, K = a.envs, 24, 64                                        # K: the stamped steps of a launch
    assert a.steps >= K
    R = K if a.old_layout else K + 1                                # stamp blocks per wave
    env = tv.VecTron(N, W, seed=0x5EED, obs_format="codes")
    env.reset()
    for _ in range(3):
        env.rollout_random(a.steps)                                 # (the stamped build leaves a totals pointer alone when it is None)
    # The buffer is sized for the largest grid the host can choose, one 64-env wave per workgroup; with four waves per
    # workgroup (256 envs) the grid is a quarter of that.  Slots nobody wrote (a workgroup past the grid, the helper wave
    # that is wave 1 of a one-wave-shape workgroup) are told by a zero first stamp and left out.
    blocks = (N + 63) // 64
    HS = 4 + 2 * (K // a.block)                                     # helper slots per stamped wave
    nh = 0 if a.old_layout else blocks * 2 * HS
    runs, hruns = [], []
    for _ in range(a.launches):
        buf = torch.zeros(blocks * 2 * R * 4 + nh, dtype=torch.int64, device="cuda")
        env.rollout_random(a.steps, buf)
        torch.cuda.synchronize()
        flat = buf.cpu().numpy()
        r = flat[:blocks * 2 * R * 4].reshape(blocks * 2, R, 4)
        runs.append(r[r[:, 0, 0] > 0].astype(np.float64) * 0.01)    # us
        if nh:
            hruns.append(flat[blocks * 2 * R * 4:].reshape(blocks * 2, HS)[r[:, 0, 0] > 0].astype(np.float64) * 0.01)
    waves = len(runs[0])
    assert waves > 0 and all(len(r) == waves for r in runs), "no stamps: is the library a -DTRON_STAMPS build?"
    t = np.stack(runs, 0)                                           # [launches, stamped waves, K, 4]

    def row(name, x):
        x = x.reshape(-1)
        print(f"  {name:44s} {np.median(x):6.2f} [{np.percentile(x, 10):6.2f} {np.percentile(x, 90):6.2f}]  mean {x.mean():6.2f}")

    phases = [("move (0->1)", 0, 1), ("restart: state, board, next starts (1->2)", 1, 2), ("records (+ Philox) (2->3)", 2, 3), ("restart + records (+ Philox) (1->3)", 1, 3),
              ("whole (0->3)", 0, 3)]
    print(f"{N} envs x {W}x{W}, {waves} stamped waves, {a.launches} launches of {a.steps} steps" + (f" (the first {K} stamped)" if a.steps > K else "") + "; us, median [p10 p90], mean")
    for label, steps in (("step 0 (first of the launch)", [0]), ("steps 1..62", list(range(1, K - 1))), ("step 63 (last: no Philox block after it)" if a.steps == K else "step 63", [K - 1])):
        print(label)
        for name, i, j in phases:
            row(name, t[:, :, steps, j] - t[:, :, steps, i])
    print("step period, start to start (0 -> 0'), steps 1..62")
    row("period", t[:, :, 2:K - 1, 0] - t[:, :, 1:K - 2, 0])
    gap = t[:, :, 1:K, 0] - t[:, :, 0:K - 1, 3]                     # gap[:, :, s - 1]: in front of step s
    first = np.arange(1, K) % a.block == 0
    row(f"gap 3 -> 0' in front of a block (s % {a.block} == 0: the barrier)", gap[:, :, first])
    row("gap 3 -> 0' inside a block", gap[:, :, ~first])
    print("phase 1->2 by step, median us:")
    med = np.median((t[:, :, :, 2] - t[:, :, :, 1]).reshape(-1, K), 0)
    print("  " + " ".join(f"{x:.2f}" for x in med))
    span = t[:, :, K - 1, 3].reshape(a.launches, -1).max(1) - t[:, :, 0, 0].reshape(a.launches, -1).min(1)
    print("launch span, first step start -> last step's last stamp (the prologue is before it): " + " ".join(f"{x:.1f}" for x in span) + " us")
    if not a.old_layout:
        print("the launch, per wave")
        row("prologue (kernel entry -> first step)", t[:, :, 0, 0] - t[:, :, K, 0])
        row("step loop (first step -> loop left)", t[:, :, K, 1] - t[:, :, 0, 0])
        if a.steps > K:
            loop = t[:, :, K, 1] - t[:, :, 0, 0]
            print(f"    per launch, p90 - p10 of the waves' loop times: " + " ".join(f"{np.percentile(x, 90) - np.percentile(x, 10):.2f}" for x in loop) + " us")
            row(f"the first {K} steps of the loop (first step -> step {K - 1}'s last stamp)", t[:, :, K - 1, 3] - t[:, :, 0, 0])
        row("epilogue: plane stores issued", t[:, :, K, 2] - t[:, :, K, 1])
        row("epilogue: state words", t[:, :, K, 3] - t[:, :, K, 2])
        whole = t[:, :, K, 3].reshape(a.launches, -1).max(1) - t[:, :, K, 0].reshape(a.launches, -1).min(1)
        print("first kernel entry -> last kernel end: " + " ".join(f"{x:.1f}" for x in whole) + " us")
    if hruns and all((h[:, 0] > 0).all() for h in hruns):
        h = np.stack(hruns, 0)                                      # [launches, stamped waves, HS]
        nb = K // a.block
        bs = np.arange(1, nb)                                       # the barriers B_1 .. B_(nb-1)
        g_arr, g_dep = t[:, :, bs * a.block - 1, 3], t[:, :, bs * a.block, 0]
        h_arr, h_dep = h[:, :, 2 + 2 * bs], h[:, :, 3 + 2 * bs]
        entry = "drawn (TRON_ROLL_NO_HANDOFF)" if os.environ.get("TRON_ROLL_NO_HANDOFF") else "handed over by the launch before"
        print(f"the helper beside its game wave; block 0's starts and actions: {entry}")
        row("helper: prologue draws (entry -> done)", h[:, :, 1] - h[:, :, 0])
        row("helper: wait at P", h[:, :, 3] - h[:, :, 2])
        row("game: entry -> arrival at P", h[:, :, HS - 1] - t[:, :, K, 0])
        row("game: wait at P (arrival -> first step)", t[:, :, 0, 0] - h[:, :, HS - 1])
        late = h[:, :, 2] - h[:, :, HS - 1]
        row("P: helper's arrival - game's", late)
        print(f"    the helper is the later one at P in {100.0 * (late > 0).mean():.0f} % of the pairs")
        row("game: block's work (release -> next arrival)", g_arr[:, :, 1:] - g_dep[:, :, :-1])
        row("helper: block's work (release -> next arrival)", h_arr[:, :, 1:] - h_dep[:, :, :-1])
        row("helper: block 0's work, its top-up (P -> arrival at B_1)", h_arr[:, :, 0] - h[:, :, 3])
        late1 = h_arr[:, :, 0] - g_arr[:, :, 0]
        row("B_1: helper's arrival - game's", late1)
        print(f"    the helper is the later one at B_1 in {100.0 * (late1 > 0).mean():.0f} % of the pairs")
        if (h[:, :, HS - 2] > 0).all() and a.steps == K:          # (a longer launch: B_(nb-1) is not among the stamped barriers)
            row("helper: hand-off pass (B_(nb-1) left -> stores issued)", h[:, :, HS - 2] - h_dep[:, :, -1])
            row("helper: hand-off pass ends before its game wave leaves the loop by", t[:, :, K, 1] - h[:, :, HS - 2])
        row("game: wait at a block barrier", g_dep - g_arr)
        row("helper: wait at a block barrier", h_dep - h_arr)
        late = h_arr - g_arr
        row("B_b: helper's arrival - game's", late)
        print(f"    the helper is the later one in {100.0 * (late > 0).mean():.0f} % of the pair-barriers; by barrier, median us: "
              + " ".join(f"{x:.2f}" for x in np.median(late.reshape(-1, nb - 1), 0)))
        # the last of the stamped waves of a workgroup (two game waves and their helpers in the four-wave shape)
        last = np.maximum(g_arr, h_arr)
        row("B_b: release - the pair's later arrival (waiting for others)", np.minimum(g_dep, h_dep) - last)
    elif not a.old_layout:
        print("no helper stamps (a library from before the helpers stamped)")


if __name__ == "__main__":
    main()
