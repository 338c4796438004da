#!/usr/bin/env python3
"""tron_territory_codes (tron.vec.territory_codes) at 262 144 boards of 12x12 and 26x26 bytes (widths 10 and 24): boards
per second and the effective bandwidth of reading the boards, on fresh boards (both floods run to the far corner) and on
soup boards (the positions after a random number of drawn steps, 0 .. W * W / 3, of playout_codes), with and without the
owner plane, and tron_minimax_codes in Voronoi mode on the same boards beside it — the only other device path that floods
(up to 16 leaves per board, each with both floods, and byte-wise board reads).

One process, the variants alternated so that they share the clocks; a window is --launches calls timed by device events;
every variant is warmed up, then --repeats rounds run the variants one after the other.  The board stack (38 MB / 177 MB)
does not fit the L2 and fits the Infinity Cache only at 12x12, so "read GB/s" is board bytes over time, whatever served
them.  Prints one line per variant (median [min max] over the rounds) and one JSON line.
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


def make_boards(n, W, soup):
    src = tv.VecTron(n, W, seed=0x5EED, rank=0)
    src.reset()
    boards = src.obs[:, 0].contiguous()
    src.close()
    if not soup:
        return boards
    # every board plays a random number of drawn steps: rounds of one step (a `call` each), taken only by the boards that
    # have not reached their length and are still live
    length = torch.randint(0, max(2, W * W // 3), (n,), device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    for t in range(int(length.max())):
        _, winner, after = tv.playout_codes(boards, None, 1, call=t, want_codes=True)
        move = ((length > t) & (winner == -1)).view(n, 1, 1)
        boards = torch.where(move, after, boards)
    return boards


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=262144)
    ap.add_argument("--widths", type=int, nargs="*", default=[10, 24])
    ap.add_argument("--launches", type=int, default=4, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2, help="warm-up windows per variant")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("territory_bench.py measures on the GPU; none here")

    n, out = a.boards, []
    for W in a.widths:
        S = W + 2
        for kind in ("fresh", "soup"):
            boards = make_boards(n, W, kind == "soup")
            counts = tv.territory_codes(boards)[0]
            ok = counts[:, 0] >= 0
            both = counts[:, 4] + counts[:, 5] - counts[:, :3].sum(1)
            print(f"{n} {kind} boards of {S}x{S}: {int(ok.sum())} playable, {int((ok & (both == 0)).sum())} of them separated, "
                  f"{float(counts[ok][:, :4].sum(1).float().mean()):.1f} open cells a board; windows of {a.launches} calls, "
                  f"{a.repeats} rounds: median [min max]")
            variants = [("territory counts", lambda: tv.territory_codes(boards)),
                        ("territory counts+owner", lambda: tv.territory_codes(boards, want_owner=True)),
                        ("minimax_codes voronoi", lambda: tv.minimax_codes(boards))]
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
                gbs = [n * S * S / (t * 1e-3) / 1e9 for t in ms[name]]
                print(f"  {name:24s} {statistics.median(ms[name]):8.3f} ms/call [{min(ms[name]):8.3f} {max(ms[name]):8.3f}]   "
                      f"{statistics.median(per_s):8.1f} M boards/s [{min(per_s):8.1f} {max(per_s):8.1f}]   "
                      f"read {statistics.median(gbs):7.1f} GB/s", flush=True)
            out.append(dict(width=W, kind=kind, ms=ms))
    print(json.dumps(dict(boards=n, launches=a.launches, results=out)))


if __name__ == "__main__":
    main()
