#!/usr/bin/env python3
"""Monte-Carlo against Monte-Carlo on one VecTron: does a weighted playout policy make the flat Monte-Carlo opponent
stronger than the uniform safe draw does?

Player 1 moves by montecarlo_actions(1, weights=A) and player 2 by montecarlo_actions(2, weights=B), with the same
`copies` and `k_steps` and call streams of their own (2t for player 1, 2t + 1 for player 2 at step t), on --games games
from fair random starts, until every game is over.  Each round (an env seed of its own) plays both seatings — A as
player 1 against B as player 2, then B as player 1 against A — and A's score of the round is (wins + draws / 2) / games
over the two.  For every candidate A in --candidates against B = None (the uniform draw), and for None against None as
the control that shows what the seats and the streams alone do, prints wins, draws and losses summed over the rounds and
the score as median [min max] over the rounds.  A candidate beats the uniform draw when its range lies above the
control's.

--mode none plays mode None; --mode ice plays "ice" at --slide with rates=True, so the playouts follow the env's rule.
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


def name(weights):
    return "None" if weights is None else "(" + ",".join(map(str, weights)) + ")"


def weights_of(text):
    return None if text.lower() == "none" else tuple(int(x) for x in text.split(","))


def play(a, env, first, second):
    """One seating: (wins of player 1, wins of player 2, draws) with `first` / `second` as the seats' weights."""
    sliding = {} if a.mode == "none" else dict(rates=True)
    env.reset()
    for t in range(a.width * a.width):
        a1 = env.montecarlo_actions(1, a.k_steps, a.copies, call=2 * t, weights=first, **sliding)
        a2 = env.montecarlo_actions(2, a.k_steps, a.copies, call=2 * t + 1, weights=second, **sliding)
        _, _, done, _ = env.step(torch.stack([a1, a2], 1), autoreset=False)
        if bool(done.all()):
            break
    winner = env.state()["winner"]
    p1, p2 = int((winner == 1).sum()), int((winner == 2).sum())
    return p1, p2, a.games - p1 - p2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["none", "ice"], default="none")
    ap.add_argument("--slide", type=float, default=0.15, help="the slide of every game in --mode ice")
    ap.add_argument("--games", type=int, default=8192)
    ap.add_argument("--width", type=int, default=10)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--k-steps", type=int, default=None, help="default: width * width")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--candidates", nargs="*", default=["1,8,4,2", "1,4,2,1", "0,4,2,1", "1,1,2,4"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("playout_policy_match.py plays on the GPU; none here")

    pairs = [(None, None)] + [(weights_of(c), None) for c in a.candidates]
    out = []
    print(f"mode {a.mode}" + ("" if a.mode == "none" else f" slide {a.slide:g}, rates=True") + f", {a.games} games of "
          f"{a.width}x{a.width} per seating, copies {a.copies}, k_steps {a.k_steps or a.width * a.width}, {a.rounds} rounds of "
          f"two seatings: A against B, A's wins / draws / losses over all rounds, A's score median [min max] over the rounds")
    for A, B in pairs:
        wins = draws = losses = 0
        scores = []
        for r in range(a.rounds):
            env = tv.VecTron(a.games, a.width, mode=None if a.mode == "none" else "ice", fair=True, seed=0x5EED + r,
                             obs_format="codes")
            if a.mode == "ice":
                env.set_slide(torch.full((a.games,), a.slide, dtype=torch.float64, device=env.device))
            p1, p2, d = play(a, env, A, B)                             # A sits as player 1
            q1, q2, e = play(a, env, B, A)                             # ... and as player 2
            env.close()
            wins, draws, losses = wins + p1 + q2, draws + d + e, losses + p2 + q1
            scores.append((p1 + q2 + 0.5 * (d + e)) / (2 * a.games))
        print(f"  {name(A):12s} against {name(B):5s} {wins:8d} / {draws:7d} / {losses:8d}   score {statistics.median(scores):.4f} "
              f"[{min(scores):.4f} {max(scores):.4f}]", flush=True)
        out.append(dict(A=A, B=B, wins=wins, draws=draws, losses=losses, scores=scores))
    print(json.dumps(dict(mode=a.mode, slide=a.slide, games=a.games, width=a.width, copies=a.copies, k_steps=a.k_steps,
                          rounds=a.rounds, results=out)))


if __name__ == "__main__":
    main()
