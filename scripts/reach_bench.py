#!/usr/bin/env python3
"""tron_reach_codes (tron.vec.reach_codes) at 262 144 boards of 12x12 and 26x26 bytes (widths 10 and 24): boards per second
for the counts alone and with both distance planes, on fresh boards (both floods run to the far corner) and on soup boards
(scripts/territory_bench.py's: the positions after a random number of drawn steps), with tron_territory_codes on the same
boards in the same run as the yardstick.  The counts-only call runs territory's flood loop and keeps no level; the call
with planes adds the bit-sliced levels, their expansion to int16 and 4 * S * S bytes of stores per board.

One process, the variants alternated so that they share the clocks; a window is --launches calls timed by device events;
every variant is warmed up, then --repeats rounds run the variants one after the other.  Prints one line per variant
(median [min max] over the rounds) and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deep-q-learning_tron_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import tron.vec as tv  # noqa: E402
from territory_bench import make_boards  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=262144)
    ap.add_argument("--widths", type=int, nargs="*", default=[10, 24])
    ap.add_argument("--launches", type=int, default=4, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up windows per variant")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reach_bench.py measures on the GPU; none here")

    n, out = a.boards, []
    for W in a.widths:
        S = W + 2
        for kind in ("fresh", "soup"):
            boards = make_boards(n, W, kind == "soup")
            counts = tv.reach_codes(boards)[0]
            ok = counts[:, 0] >= 0
            print(f"{n} {kind} boards of {S}x{S}: {int(ok.sum())} playable, depth {float(counts[ok][:, 6:].float().mean()):.1f} mean / "
                  f"{int(counts[:, 6:].max())} max; windows of {a.launches} calls, {a.repeats} rounds: median [min max]")
            variants = [("territory counts", lambda: tv.territory_codes(boards)),
                        ("territory counts+owner", lambda: tv.territory_codes(boards, want_owner=True)),
                        ("reach counts", lambda: tv.reach_codes(boards)),
                        ("reach counts+planes", lambda: tv.reach_codes(boards, want_dist=True))]
            for _, fn in variants:
                for _ in range(a.warmup * a.launches):
                    fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _ in variants}
            for _ in range(a.repeats):
                for name, fn in variants:
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.launches):
                        fn()
                    t1.record()
                    t1.synchronize()
                    ms[name].append(t0.elapsed_time(t1) / a.launches)
            for name, _ in variants:
                per_s = [n / (t * 1e-3) / 1e6 for t in ms[name]]
                print(f"  {name:24s} {statistics.median(ms[name]):8.3f} ms/call [{min(ms[name]):8.3f} {max(ms[name]):8.3f}]   "
                      f"{statistics.median(per_s):8.1f} M boards/s [{min(per_s):8.1f} {max(per_s):8.1f}]", flush=True)
            out.append(dict(width=W, kind=kind, ms=ms))
    print(json.dumps(dict(boards=n, launches=a.launches, results=out)))


if __name__ == "__main__":
    main()
