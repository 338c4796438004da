#!/usr/bin/env python3
"""Short territory-judged playouts against full-length playouts, Monte-Carlo against Monte-Carlo on one VecTron in mode
None (scripts/playout_policy_match.py's frame).

Candidate A moves by montecarlo_actions(judge="territory", k_steps=k) for every k in --k-steps: 16 * copies playouts of at
most k steps, those that k cuts off judged by who reaches more cells first.  The opponent B is the full-length uniform
Monte-Carlo player, montecarlo_actions(k_steps=width * width) with the same copies.  The seats draw from call streams of
their own (2t for player 1, 2t + 1 for player 2 at step t), on --games games from fair random starts, until every game is
over.  Each round (an env seed of its own) plays both seatings and A's score of the round is (wins + draws / 2) / games
over the two.  The control is B against itself: what the seats and the streams alone do.  Prints wins, draws and losses
summed over the rounds, the score as median [min max] over the rounds, and the time of one move of either opponent (one
montecarlo_actions call for all games, device events, median over all moves of all rounds).  A candidate beats the
full-length player when its range lies above the control's.
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


def name(k):
    return "full" if k is None else f"judged k={k}"


def play(a, env, first, second, times):
    """One seating: (wins of player 1, wins of player 2, draws); first / second: the seats' k (None: full length)."""
    env.reset()
    events = []
    for t in range(a.width * a.width):
        acts = []
        for player, k in ((1, first), (2, second)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            acts.append(env.montecarlo_actions(player, a.width * a.width if k is None else k, a.copies, call=2 * t + player - 1,
                                               judge=None if k is None else "territory"))
            t1.record()
            events.append((k, t0, t1))
        _, _, done, _ = env.step(torch.stack(acts, 1), autoreset=False)
        if bool(done.all()):
            break
    torch.cuda.synchronize()
    for k, t0, t1 in events:
        times.setdefault(k, []).append(t0.elapsed_time(t1))
    winner = env.state()["winner"]
    p1, p2 = int((winner == 1).sum()), int((winner == 2).sum())
    return p1, p2, a.games - p1 - p2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--width", type=int, default=10)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--k-steps", type=int, nargs="*", default=None, help="default: 1, width / 2, width, 2 * width")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("territory_policy_match.py plays on the GPU; none here")
    ks = a.k_steps or [1, a.width // 2, a.width, 2 * a.width]

    out, times = [], {}
    print(f"mode none, {a.games} games of {a.width}x{a.width} per seating, copies {a.copies}, {a.rounds} rounds of two seatings: A "
          f"against B = full-length uniform playouts (k_steps {a.width * a.width}); A's wins / draws / losses over all rounds, "
          f"A's score median [min max] over the rounds")
    for A in [None] + ks:
        wins = draws = losses = 0
        scores = []
        for r in range(a.rounds):
            env = tv.VecTron(a.games, a.width, mode=None, fair=True, seed=0x5EED + r, obs_format="codes")
            p1, p2, d = play(a, env, A, None, times)                   # A sits as player 1
            q1, q2, e = play(a, env, None, A, times)                   # ... and as player 2
            env.close()
            wins, draws, losses = wins + p1 + q2, draws + d + e, losses + p2 + q1
            scores.append((p1 + q2 + 0.5 * (d + e)) / (2 * a.games))
        print(f"  {name(A):12s} against full {wins:8d} / {draws:7d} / {losses:8d}   score {statistics.median(scores):.4f} "
              f"[{min(scores):.4f} {max(scores):.4f}]", flush=True)
        out.append(dict(A=A, wins=wins, draws=draws, losses=losses, scores=scores))
    print(f"one move for all {a.games} games (median over all moves, ms):")
    for k in [None] + ks:
        print(f"  {name(k):12s} {statistics.median(times[k]):8.3f} ms   ({len(times[k])} moves)")
    print(json.dumps(dict(games=a.games, width=a.width, copies=a.copies, rounds=a.rounds, results=out,
                          move_ms={name(k): statistics.median(v) for k, v in times.items()})))


if __name__ == "__main__":
    main()
