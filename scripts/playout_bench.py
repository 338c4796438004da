#!/usr/bin/env python3
"""Rates of tron_playout_codes (tron.vec.playout_codes) at 65 536 fresh 24x24 boards x 4 copies, k_steps = 128, with
VecTron.rollout_actions at the same number of envs and steps beside it; one process, the variants alternated so that they
share the clocks:

  drawn    actions=None: every move a safe draw (four LDS reads per player and a Philox block per playout-step)
  tape     a full tape of random actions 0..3 (2 bytes read per playout-step); these games end after a few steps
  rollout  VecTron.rollout_actions: --playouts live envs with autoreset under the same tape, one persistent launch

A window is --launches launches, each with its own `call` (so the drawn playouts differ from launch to launch), timed by
device events; every variant is warmed up, then --repeats rounds run the variants one after the other.  A playout
variant's steps are the steps actually played, out_steps summed over the window's launches; the rollout's are envs x
steps (a finished env restarts and plays on).  Prints one line per variant (median [min max] over the rounds) and one
JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-q-learning_tron_amd"))

import torch  # noqa: E402
import tron.vec as tv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--width", type=int, default=24)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--launches", type=int, default=8, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3, help="warm-up windows per variant")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("playout_bench.py measures on the GPU; none here")

    n, K = a.boards * a.copies, a.steps
    src = tv.VecTron(a.boards, a.width, seed=0x5EED, rank=0)
    src.reset()
    boards = src.obs[:, 0].repeat_interleave(a.copies, dim=0)          # what VecTron.playout(copies=...) plays
    src.close()
    tape = torch.randint(0, 4, (K, n, 2), dtype=torch.int8, device="cuda")
    env = tv.VecTron(n, a.width, seed=0x5EED, rank=0)
    assert env.obs_is_state
    env.reset()
    calls = [0]

    def run_playouts(actions):
        def run():
            steps = []
            for _ in range(a.launches):
                calls[0] += 1
                steps.append(tv.playout_codes(boards, actions, K, call=calls[0])[0])
            return lambda: sum(int(s.sum()) for s in steps)            # read back after the window
        return run

    def run_rollout():
        for _ in range(a.launches):
            env.rollout_actions(tape)
        return lambda: a.launches * n * K

    variants = [("drawn", run_playouts(None)), ("tape", run_playouts(tape)), ("rollout", run_rollout)]
    for _, fn in variants:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in variants}
    steps = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, fn in variants:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            count = fn()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
            steps[name].append(count())
    print(f"{n} playouts ({a.boards} fresh {a.width}x{a.width} boards x {a.copies}), k_steps {K}, windows of {a.launches} launches, "
          f"{a.repeats} rounds: median [min max]")
    for name, _ in variants:
        per_launch = [t / a.launches for t in ms[name]]
        rate = [s / (t * 1e-3) / 1e9 for s, t in zip(steps[name], ms[name])]
        line = (f"  {name:8s} {statistics.median(per_launch):8.3f} ms/launch [{min(per_launch):8.3f} {max(per_launch):8.3f}]   "
                f"{statistics.median(rate):7.3f} G env-steps/s [{min(rate):7.3f} {max(rate):7.3f}]   "
                f"{statistics.median(steps[name]) / (a.launches * n):6.2f} steps per playout")
        if name != "rollout":
            per_s = [a.launches * n / (t * 1e-3) / 1e6 for t in ms[name]]
            line += f"   {statistics.median(per_s):8.2f} M playouts/s [{min(per_s):8.2f} {max(per_s):8.2f}]"
        print(line, flush=True)
    print(json.dumps({"playouts": n, "width": a.width, "k_steps": K, "launches": a.launches, "ms": ms, "steps": steps}))
    env.close()


if __name__ == "__main__":
    main()
