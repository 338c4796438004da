#!/usr/bin/env python3
"""tron_playout_values (tron.vec.playout_values) against the composition it replaces, at 65 536 fresh 24x24 boards, copies
4, k_steps 128; one process, the variants alternated so that they share the clocks:

  values    playout_values(boards, k_steps, copies): counts, steps and actions from the 44 MB of boards
  composed  repeat_interleave of the boards 16 * copies times, a step-major tape whose first row holds the moves and whose
            other rows are negative, playout_codes, and scatter_add of the winners and steps per board and move — all of
            it inside the timed window, as a caller would have to run it every time the boards change

A window is --launches calls, each with its own `call`, timed by device events; every variant is warmed up, then --repeats
rounds run the variants one after the other.  Both variants play the same playouts (same key, same index), so their
tallies are compared once before the timing starts.  Prints one line per variant (median [min max] over the rounds), the
steps per playout, and one JSON line.
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
    ap.add_argument("--launches", type=int, default=2, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up windows per variant")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("playout_values_bench.py measures on the GPU; none here")

    n, K, copies = a.boards, a.steps, a.copies
    nq = n * 16 * copies
    src = tv.VecTron(n, a.width, seed=0x5EED, rank=0)
    src.reset()
    boards = src.obs[:, 0].contiguous()
    src.close()

    def values(call):
        counts, steps, _ = tv.playout_values(boards, K, copies, call=call, want_actions=True)
        return counts, steps

    def composed(call):
        q = torch.arange(nq, device="cuda")
        move = (q // copies) % 16
        tape = torch.full((K, nq, 2), -1, dtype=torch.int8, device="cuda")
        tape[0, :, 0] = (move >> 2).to(torch.int8)
        tape[0, :, 1] = (move & 3).to(torch.int8)
        steps, winner, _ = tv.playout_codes(boards.repeat_interleave(16 * copies, dim=0), tape, K, call=call)
        at = q // copies                                               # (board, move)
        played = (winner != -2).to(torch.int32)
        counts = torch.zeros(n * 16 * 4, dtype=torch.int32, device="cuda")
        counts.scatter_add_(0, at * 4 + (winner.to(torch.int64) & 3), played)
        total = torch.zeros(n * 16, dtype=torch.int32, device="cuda")
        total.scatter_add_(0, at, steps)
        return counts.view(n, 4, 4, 4), total.view(n, 4, 4)

    for x, y in zip(values(1), composed(1)):
        assert torch.equal(x, y), "the two variants disagree"
    calls = [1]

    def window(fn):
        def run():
            out = []
            for _ in range(a.launches):
                calls[0] += 1
                out.append(fn(calls[0])[1])
            return lambda: sum(int(s.sum()) for s in out)              # read back after the window
        return run

    variants = [("values", window(values)), ("composed", window(composed))]
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
    print(f"{nq} playouts ({n} fresh {a.width}x{a.width} boards x 16 first moves x {copies}), k_steps {K}, windows of "
          f"{a.launches} calls, {a.repeats} rounds: median [min max]")
    for name, _ in variants:
        per_call = [t / a.launches for t in ms[name]]
        per_s = [a.launches * nq / (t * 1e-3) / 1e6 for t in ms[name]]
        print(f"  {name:9s} {statistics.median(per_call):9.3f} ms/call [{min(per_call):9.3f} {max(per_call):9.3f}]   "
              f"{statistics.median(per_s):8.2f} M playouts/s [{min(per_s):8.2f} {max(per_s):8.2f}]   "
              f"{statistics.median(steps[name]) / (a.launches * nq):6.2f} steps per playout", flush=True)
    print(json.dumps({"boards": n, "copies": copies, "width": a.width, "k_steps": K, "launches": a.launches, "ms": ms,
                      "steps": steps}))


if __name__ == "__main__":
    main()
