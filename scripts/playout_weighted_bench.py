#!/usr/bin/env python3
"""Cost of the weighted safe draw beside the uniform one, one process, the variants alternated so that they share the
clocks.  Two workloads, as playout_slide_bench.py:

  codes    tron.vec.playout_codes at 262 144 fresh 24x24 boards (65 536 x 4 copies), k_steps 128, every move drawn
  values   tron.vec.playout_values at 65 536 fresh 24x24 boards x copies 4 (4 194 304 playouts), k_steps 128

each with weights=None (tron_playout_codes / tron_playout_values), with (1,1,1,1) — the same games through the weighted
kernels — and with tron.vec.HUG_WEIGHTS, whose games are other games: the steps per playout stand beside every time.
--rate R times all of it under the sliding rule at rate R for both players instead.

A window is --launches calls, each with its own `call`, timed by device events; every variant is warmed up, then
--repeats rounds run the variants one after the other.  Prints one line per variant (median [min max] over the rounds)
and one JSON line.
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
    ap.add_argument("--rate", type=float, default=None, help="play the sliding rule at this rate for both players")
    ap.add_argument("--launches", type=int, default=2, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up windows per variant")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("playout_weighted_bench.py measures on the GPU; none here")

    n, K, copies = a.boards, a.steps, a.copies
    src = tv.VecTron(n, a.width, seed=0x5EED, rank=0)
    src.reset()
    boards = src.obs[:, 0].contiguous()
    src.close()
    forks = boards.repeat_interleave(copies, dim=0)                    # what VecTron.playout(copies=...) plays
    rates = {m: {} if a.rate is None else dict(rates=torch.full((m, 2), a.rate, dtype=torch.float64, device="cuda"))
             for m in (n, len(forks))}
    calls = [0]

    def window(fn):
        def run():
            steps = []
            for _ in range(a.launches):
                calls[0] += 1
                steps.append(fn(calls[0]))
            return lambda: sum(int(s.sum()) for s in steps)            # read back after the window
        return run

    def codes(weights):
        return window(lambda call: tv.playout_codes(forks, None, K, call=call, weights=weights, **rates[len(forks)])[0])

    def values(weights):
        return window(lambda call: tv.playout_values(boards, K, copies, call=call, weights=weights, **rates[n])[1])

    sets = [("weights None", None), ("(1,1,1,1)", (1, 1, 1, 1)), (f"HUG {tv.HUG_WEIGHTS}".replace(" ", ""), tv.HUG_WEIGHTS)]
    variants = [(f"codes  {name}", codes(w), len(forks)) for name, w in sets]
    variants += [(f"values {name}", values(w), n * 16 * copies) for name, w in sets]
    for _, fn, _ in variants:
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in variants}
    steps = {name: [] for name, _, _ in variants}
    for _ in range(a.repeats):
        for name, fn, _ in variants:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            count = fn()
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1))
            steps[name].append(count())
    rule = "mode None's rule" if a.rate is None else f"sliding rule at rate {a.rate:g}"
    print(f"{n} fresh {a.width}x{a.width} boards, copies {copies}, k_steps {K}, {rule}, windows of {a.launches} calls, "
          f"{a.repeats} rounds: median [min max]")
    for name, _, playouts in variants:
        per_call = [t / a.launches for t in ms[name]]
        per_step = [t * 1e9 / s for t, s in zip(ms[name], steps[name])]    # ms -> ps, per playout-step
        print(f"  {name:22s} {statistics.median(per_call):9.3f} ms/call [{min(per_call):9.3f} {max(per_call):9.3f}]   "
              f"{statistics.median(steps[name]) / (a.launches * playouts):6.2f} steps per playout   "
              f"{statistics.median(per_step):7.2f} ps per playout-step [{min(per_step):7.2f} {max(per_step):7.2f}]", flush=True)
    print(json.dumps({"boards": n, "copies": copies, "width": a.width, "k_steps": K, "rate": a.rate, "launches": a.launches,
                      "ms": ms, "steps": steps}))


if __name__ == "__main__":
    main()
