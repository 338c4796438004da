#!/usr/bin/env python3
"""The maximin search seat (VecTron.search_actions: tron_search_codes' pick at 1, 2 and 3 plies, territory at the leaves)
against three opponents on one VecTron in mode None (scripts/lookahead_policy_match.py's frame and control):

  minimax    minimax_actions: MinimaxPlayer(2, "voronoi")
  lookahead  lookahead_actions: tron_moves_codes' pick
  territory  montecarlo_actions(k_steps=--k-steps, judge="territory"): short playouts judged by territory

The Monte-Carlo seat draws from call streams of its own (2t for player 1, 2t + 1 for player 2 at step t); the search, the
lookahead and the minimax draw nothing (the minimax breaks its ties by a draw of the env's own).  --games games from fair
random starts, until every game is over.  Each round (an env seed of its own) plays both seatings and A's score of the
round is (wins + draws / 2) / games over the two.  The control of an opponent is that opponent against itself: what the
seats and the streams alone do.  Prints wins, draws and losses summed over the rounds, the score as median [min max] over
the rounds, and the time of one move of every kind of seat (one call for all games, device events, median over all
moves).  A search seat beats an opponent when its range lies above the control's.
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

OPPONENTS = ("minimax", "lookahead", "territory")
SEARCHES = ("search1", "search2", "search3")


def move(a, env, seat, player, call):
    if seat in SEARCHES:
        return env.search_actions(player, plies=int(seat[-1]))
    if seat == "lookahead":
        return env.lookahead_actions(player)
    if seat == "minimax":
        return env.minimax_actions(player)
    return env.montecarlo_actions(player, a.k_steps, a.copies, call=call, judge="territory")


def play(a, env, first, second, times):
    """One seating: (wins of player 1, wins of player 2, draws); first / second: the seats' names."""
    env.reset()
    events = []
    for t in range(a.width * a.width):
        acts = []
        for player, seat in ((1, first), (2, second)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            acts.append(move(a, env, seat, player, 2 * t + player - 1))
            t1.record()
            events.append((seat, t0, t1))
        _, _, done, _ = env.step(torch.stack(acts, 1), autoreset=False)
        if bool(done.all()):
            break
    torch.cuda.synchronize()
    for seat, t0, t1 in events:
        times.setdefault(seat, []).append(t0.elapsed_time(t1))
    winner = env.state()["winner"]
    p1, p2 = int((winner == 1).sum()), int((winner == 2).sum())
    return p1, p2, a.games - p1 - p2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--width", type=int, default=10)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--k-steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("search_policy_match.py plays on the GPU; none here")

    out, times = [], {}
    print(f"mode none, {a.games} games of {a.width}x{a.width} per seating, copies {a.copies}, k_steps {a.k_steps} (territory seat), "
          f"{a.rounds} rounds of two seatings: A against B; A's wins / draws / losses over all rounds, A's score median "
          f"[min max] over the rounds")
    for B in OPPONENTS:
        for A in (B,) + SEARCHES:
            wins = draws = losses = 0
            scores = []
            for r in range(a.rounds):
                env = tv.VecTron(a.games, a.width, mode=None, fair=True, seed=0x5EED + r, obs_format="codes")
                p1, p2, d = play(a, env, A, B, times)                  # A sits as player 1
                q1, q2, e = play(a, env, B, A, times)                  # ... and as player 2
                env.close()
                wins, draws, losses = wins + p1 + q2, draws + d + e, losses + p2 + q1
                scores.append((p1 + q2 + 0.5 * (d + e)) / (2 * a.games))
            print(f"  {A:10s} against {B:10s} {wins:8d} / {draws:7d} / {losses:8d}   score {statistics.median(scores):.4f} "
                  f"[{min(scores):.4f} {max(scores):.4f}]", flush=True)
            out.append(dict(A=A, B=B, wins=wins, draws=draws, losses=losses, scores=scores))
    print(f"one move for all {a.games} games (median over all moves, ms):")
    for seat in SEARCHES + OPPONENTS:
        print(f"  {seat:10s} {statistics.median(times[seat]):8.3f} ms   ({len(times[seat])} moves)")
    print(json.dumps(dict(games=a.games, width=a.width, copies=a.copies, k_steps=a.k_steps, rounds=a.rounds, results=out,
                          move_ms={s: statistics.median(v) for s, v in times.items()})))


if __name__ == "__main__":
    main()
