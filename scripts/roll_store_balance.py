#!/usr/bin/env python3
"""How unbalanced is k_obs_roll's store loop?  A CPU estimate from the oracle, no GPU (development tool).

roll_resident (csrc/tron_env.hip) keeps one env per lane, and a step's store loop runs as many trips as the wave's slowest
lane has chunks to store.  This script steps oracle.VecOracle under autoreset and rebuilds, per env and step, the set of
16-cell chunks the kernel stores, by the mask rules in the comment above roll_resident:
  * an env that goes on stores the chunks of its move's four cells (the two old heads, the two new ones);
  * an env that finishes restarts in the same step and stores mask | the chunks of its two new heads, where mask is the set of
    chunks of its board that differ from the fresh-board template before the move (the move's own cells are not written);
  * the plane's short last chunk (G % 16 cells) is stored by a branch of its own before the loop and is counted apart.
Both planes of a chunk go out in the same trip, so a trip is one chunk.  Per wave of 64 consecutive envs and step it prints the
distribution of max (the trips the loop runs today), ceil(sum / 64) (the trips of a balanced wave-wide list) and their ratio.
usage: roll_store_balance.py [--envs N] [--width W] [--steps K] [--settle S] [--nonreversing]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    import oracle                                               # the repository's CPU oracle (ROOT/oracle)

    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--width", type=int, default=24)
    ap.add_argument("--steps", type=int, default=200, help="steps that are counted")
    ap.add_argument("--settle", type=int, default=100, help="steps before them (episode lengths reach their steady mix)")
    ap.add_argument("--nonreversing", action="store_true")
    a = ap.parse_args()

    N, W = a.envs, a.width
    S = W + 2
    G = S * S
    cpe = (G + 15) // 16
    tail = G % 16
    EMPTY, WALL = 0, -1                                             # raw tile values (map.py)
    fresh = np.full((S, S), EMPTY, np.int8)
    fresh[0, :] = fresh[-1, :] = fresh[:, 0] = fresh[:, -1] = WALL
    fresh = fresh.reshape(-1)

    oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
    v = oracle.VecOracle(N, W, seed=0x5EED)
    v.reset_all()

    def chunks(diff):
        """[N, G] bool -> [N, cpe] bool: the chunks with a marked cell."""
        pad = np.zeros((diff.shape[0], cpe * 16), bool)
        pad[:, :G] = diff
        return pad.reshape(-1, cpe, 16).any(2)

    nw = (N + 63) // 64
    mx_all, bal_all, tails, restarts, per_env, stored = [], [], 0, 0, 0, 0
    for s in range(a.settle + a.steps):
        before = v.grid.copy()
        _, d, _, _ = v.step(None, autoreset=True, want_obs=False, nonreversing=a.nonreversing)
        if s < a.settle:
            continue
        fin = d == 1
        moved = chunks(before != v.grid)                            # an env that goes on: its move's cells, all of which change
        mask = chunks(before != fresh)
        heads = chunks(v.grid != fresh)                             # after a restart: the two new heads
        sm = np.where(fin[:, None], mask | heads, moved)
        if tail:
            tails += int(sm[:, cpe - 1].sum())
            sm[:, cpe - 1] = False
        n = sm.sum(1)
        restarts += int(fin.sum())
        per_env += N
        stored += int(n.sum())
        pad = np.zeros(nw * 64, np.int64)
        pad[:N] = n
        pw = pad.reshape(nw, 64)
        mx_all.append(pw.max(1))
        bal_all.append((pw.sum(1) + 63) // 64)

    mx = np.concatenate(mx_all)
    bal = np.concatenate(bal_all)
    ratio = mx / np.maximum(bal, 1)
    q = [1, 10, 25, 50, 75, 90, 99]
    print(f"{N} envs x {W}x{W}, cpe {cpe}, tail chunk of {tail} cells, {a.steps} steps after {a.settle}, "
          f"actions {'nonreversing' if a.nonreversing else 'uniform'}; {nw} waves of 64 envs")
    print(f"restarts per env-step {restarts / per_env:.3f}; chunks per env-step in the loop {stored / per_env:.2f} "
          f"(x 2 planes = {2 * stored / per_env:.2f} 16-byte stores); tail-chunk stores per env-step {tails / per_env:.4f}")
    print("percentile            " + " ".join(f"{p:6d}" for p in q))
    print("max trips (today)     " + " ".join(f"{x:6.0f}" for x in np.percentile(mx, q)) + f"   mean {mx.mean():.2f}")
    print("ceil(sum / 64)        " + " ".join(f"{x:6.0f}" for x in np.percentile(bal, q)) + f"   mean {bal.mean():.2f}")
    print("ratio max / balanced  " + " ".join(f"{x:6.2f}" for x in np.percentile(ratio, q)) + f"   mean {ratio.mean():.2f}")
    print(f"waves with no chunk to store (T = 0): {int((bal == 0).sum())} of {len(bal)}")


if __name__ == "__main__":
    main()
