#!/usr/bin/env python3
"""tron_search_codes (tron.vec.search_codes) at soup boards of 12x12 and 26x26 bytes (widths 10 and 24;
scripts/territory_bench.py's boards: the positions after a random number of drawn steps): boards per second at 1, 2 and 3
plies, values and actions both written, with tron_moves_codes on the same boards in the same run as the yardstick.  A
search of p plies floods at most 16 ** p leaves of two fronts each where moves runs ten floods, and skips the joint moves
no board of a wave plays on.

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
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--widths", type=int, nargs="*", default=[10, 24])
    ap.add_argument("--launches", type=int, default=2, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1, help="warm-up windows per variant")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("search_bench.py measures on the GPU; none here")

    nat = tv.nat
    n, out = a.boards, []
    for W in a.widths:
        S = W + 2
        boards = make_boards(n, W, True)
        moves, actions = tv.moves_codes(boards)
        values = tv.search_codes(boards, plies=1)[0]
        ok = values[:, 0, 0] != tv.SEARCH_REJECTED
        safe = tv.safe_moves(moves)[ok].sum(-1).float().mean()
        print(f"{n} soup boards of {S}x{S}: {int(ok.sum())} playable, {float(safe):.2f} safe moves per player; windows of "
              f"{a.launches} calls, {a.repeats} rounds: median [min max]")
        cp, mp, vp, ap_, st = nat.ptr(boards), nat.ptr(moves), nat.ptr(values), nat.ptr(actions), nat.stream_ptr()
        L = nat.lib()
        variants = [("moves + actions", lambda: L.tron_moves_codes(cp, n, S, mp, ap_, st))]
        for plies in (1, 2, 3):
            variants.append((f"search {plies} plies", lambda plies=plies: L.tron_search_codes(cp, n, S, plies, vp, ap_, st)))
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
            print(f"  {name:16s} {statistics.median(ms[name]):9.3f} ms/call [{min(ms[name]):9.3f} {max(ms[name]):9.3f}]   "
                  f"{statistics.median(per_s):9.3f} M boards/s [{min(per_s):9.3f} {max(per_s):9.3f}]", flush=True)
        out.append(dict(width=W, ms=ms))
    print(json.dumps(dict(boards=n, launches=a.launches, results=out)))


if __name__ == "__main__":
    main()
