#!/usr/bin/env python3
"""tron_moves_codes (tron.vec.moves_codes) at 262 144 soup boards of 12x12 and 26x26 bytes (widths 10 and 24;
scripts/territory_bench.py's boards: the positions after a random number of drawn steps): boards per second for the moves
alone, the actions alone and both, with tron_reach_codes' counts on the same boards in the same run as the yardstick.  The
kernel runs ten floods per board where reach runs two, so five times reach's time is what the floods alone would cost; the
last line of each block is the measured ratio.

The entries are called on outputs allocated once, so a window holds launches and nothing else.  One process, the variants
alternated so that they share the clocks; a window is --launches calls timed by device events; every variant is warmed up,
then --repeats rounds run the variants one after the other.  Prints one line per variant (median [min max] over the
rounds) and one JSON line.
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
        sys.exit("moves_bench.py measures on the GPU; none here")

    nat = tv.nat
    n, out = a.boards, []
    for W in a.widths:
        S = W + 2
        boards = make_boards(n, W, True)
        moves, actions = tv.moves_codes(boards)
        counts = tv.reach_codes(boards)[0]
        ok = counts[:, 0] >= 0
        safe = tv.safe_moves(moves)[ok].sum(-1).float().mean()
        print(f"{n} soup boards of {S}x{S}: {int(ok.sum())} playable, {float(safe):.2f} safe moves per player, reach depth "
              f"{float(counts[ok][:, 6:].float().mean()):.1f} mean / {int(counts[:, 6:].max())} max; windows of {a.launches} calls, "
              f"{a.repeats} rounds: median [min max]")
        cp, mp, ap_, rp, st = nat.ptr(boards), nat.ptr(moves), nat.ptr(actions), nat.ptr(counts), nat.stream_ptr()
        L = nat.lib()
        variants = [("reach counts", lambda: L.tron_reach_codes(cp, n, S, rp, None, st)),
                    ("moves only", lambda: L.tron_moves_codes(cp, n, S, mp, None, st)),
                    ("actions only", lambda: L.tron_moves_codes(cp, n, S, None, ap_, st)),
                    ("moves + actions", lambda: L.tron_moves_codes(cp, n, S, mp, ap_, st))]
        for _, fn in variants:
            for _ in range(a.warmup * a.launches):
                assert fn() == nat.OK
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
            print(f"  {name:16s} {statistics.median(ms[name]):8.3f} ms/call [{min(ms[name]):8.3f} {max(ms[name]):8.3f}]   "
                  f"{statistics.median(per_s):8.1f} M boards/s [{min(per_s):8.1f} {max(per_s):8.1f}]", flush=True)
        ratio = statistics.median(ms["moves + actions"]) / statistics.median(ms["reach counts"])
        print(f"  moves + actions / reach counts = {ratio:.2f} (ten floods to two: 5.00)")
        out.append(dict(width=W, ms=ms, ratio=ratio))
    print(json.dumps(dict(boards=n, launches=a.launches, results=out)))


if __name__ == "__main__":
    main()
