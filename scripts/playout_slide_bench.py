#!/usr/bin/env python3
"""Rates of the sliding playout kernels beside the mode-None ones, one process, the variants alternated so that they
share the clocks.  Two workloads:

  codes    tron.vec.playout_codes at 262 144 fresh 24x24 boards (65 536 x 4 copies), k_steps 128, every move drawn
  values   tron.vec.playout_values at 65 536 fresh 24x24 boards x copies 4 (4 194 304 playouts), k_steps 128

each as `none` (rates=None: tron_playout_codes / tron_playout_values) and under the sliding rule with both players' rates
0, 0.15 and 0.5 on every board (tron_playout_slide_codes / tron_playout_slide_values, drawn uniforms).

A window is --launches calls, each with its own `call`, timed by device events; every variant is warmed up, then
--repeats rounds run the variants one after the other.  Prints one line per variant (median [min max] over the rounds)
with the steps per playout, and one JSON line.

--pkg DIR imports the package from another tree and --none-only times the `none` variants alone: together they time an
older tree's mode-None kernels from fresh processes, to be alternated with this tree's (profiles/README.md).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--width", type=int, default=24)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rates", type=float, nargs="*", default=[0.0, 0.15, 0.5])
    ap.add_argument("--launches", type=int, default=2, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up windows per variant")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "deep-q-learning_tron_amd"), help="the package directory to import")
    ap.add_argument("--none-only", action="store_true", help="time the mode-None entries alone")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg))
    import torch
    import tron.vec as tv
    if not torch.cuda.is_available():
        sys.exit("playout_slide_bench.py measures on the GPU; none here")

    n, K, copies = a.boards, a.steps, a.copies
    src = tv.VecTron(n, a.width, seed=0x5EED, rank=0)
    src.reset()
    boards = src.obs[:, 0].contiguous()
    src.close()
    forks = boards.repeat_interleave(copies, dim=0)                    # what VecTron.playout(copies=...) plays
    calls = [0]

    def window(fn):
        def run():
            steps = []
            for _ in range(a.launches):
                calls[0] += 1
                steps.append(fn(calls[0]))
            return lambda: sum(int(s.sum()) for s in steps)            # read back after the window
        return run

    def codes(rate):
        kw = {} if rate is None else dict(rates=torch.full((len(forks), 2), rate, dtype=torch.float64, device="cuda"))
        return window(lambda call: tv.playout_codes(forks, None, K, call=call, **kw)[0])

    def values(rate):
        kw = {} if rate is None else dict(rates=torch.full((n, 2), rate, dtype=torch.float64, device="cuda"))
        return window(lambda call: tv.playout_values(boards, K, copies, call=call, **kw)[1])

    rates = [None] + ([] if a.none_only else list(a.rates))
    label = lambda rate: "none" if rate is None else f"rate {rate:g}"
    variants = [(f"codes  {label(r)}", codes(r), len(forks)) for r in rates]
    variants += [(f"values {label(r)}", values(r), n * 16 * copies) for r in rates]
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
    print(f"{n} fresh {a.width}x{a.width} boards, copies {copies}, k_steps {K}, windows of {a.launches} calls, {a.repeats} rounds: "
          f"median [min max]")
    for name, _, playouts in variants:
        per_call = [t / a.launches for t in ms[name]]
        per_s = [a.launches * playouts / (t * 1e-3) / 1e6 for t in ms[name]]
        print(f"  {name:17s} {statistics.median(per_call):9.3f} ms/call [{min(per_call):9.3f} {max(per_call):9.3f}]   "
              f"{statistics.median(per_s):8.2f} M playouts/s [{min(per_s):8.2f} {max(per_s):8.2f}]   "
              f"{statistics.median(steps[name]) / (a.launches * playouts):6.2f} steps per playout", flush=True)
    print(json.dumps({"boards": n, "copies": copies, "width": a.width, "k_steps": K, "launches": a.launches, "ms": ms,
                      "steps": steps}))


if __name__ == "__main__":
    main()
