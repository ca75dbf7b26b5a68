#!/usr/bin/env python3
"""Gumbel self-play with the exact solver's guard, in one launch per window (``gbl_collect_gumbel_solve``), on the host flavour by
default.  ``search=dict(iterations=16, gumbel=dict(considered=16, solve_depth=3))``: before every search the solver looks 3 plies
ahead; a root it proves plays the proven move ("how" = ``nat.HOW_PROVEN``, a one-hot policy row, no noise drawn), every other root runs
the 16-iteration Gumbel search over the moves the solver left unproven ("how" = ``nat.HOW_GUMBEL``, the completed-Q row as the target).
Both kinds of ply are training rows.  A few windows of evaluator against evaluator (an untrained seeded network) go through
``outcome_targets`` into a ReplayBuffer and a short fit, guarded and unguarded from the same boards and seed; then a small arena on
fresh boards, the guarded side against the unguarded one as either colour.
    python examples/example_gumbel_guarded.py [device] [--boards N] [--plies T] [--windows W] [--depth D] [--steps S]
One seed, no claim beyond the printed lines."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
from example_gumbel import seeded_evaluator  # noqa: E402


def windows(device, gumbel, boards, plies, count, steps, seed=1):
    """`count` windows of `plies` plies with ``gumbel=``, appended and fitted: the rows kept, the plies by `how` code, the share of
    guarded plies the solver proved, and the fit's last (policy loss, value loss)."""
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    buf = G.ReplayBuffer(boards * plies * count, device)
    search = dict(evaluator=seeded_evaluator(device), iterations=16, gumbel=gumbel)
    kinds, proven, solved = {}, 0, 0
    for w in range(count):
        tr = env.collect(plies, policies=("evaluator", "evaluator"), search=search)
        env.outcome_targets(tr)
        buf.append(env, tr, tag=w)
        for code, n in zip(*np.unique(tr["how"].cpu().numpy(), return_counts=True)):
            kinds[int(code)] = kinds.get(int(code), 0) + int(n)
        if "proven" in tr:  # (the guard's two arrays: only a guarded window has them)
            proven += int((tr["proven"] != 0).sum())
            solved += int((tr["outcomes"] != nat.SOLVE_NONE).any(-1).sum())
    stats = buf.fit(G.GobbletTrainer(64, device, seed=0), steps, batch=512, symmetries=None)
    return buf.total, kinds, proven / max(solved, 1), (float(stats[-1, 0]), float(stats[-1, 1]))


def arena(device, depth, games=64, plies=64, seed=11):
    """The guarded side against the unguarded one, both Gumbel at 16 iterations with the same network, as either colour: (wins, losses)
    of the guarded side over the first finished game of every board."""
    ev, wins, losses = seeded_evaluator(device), 0, 0
    for guarded in (0, 1):
        env = G.BatchedGobblet(games, device, auto_reset=True, seed=seed, track_turn=True)
        deps = (depth, 0) if guarded == 0 else (0, depth)
        tr = env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=16, gumbel=dict(considered=16, solve_depth=deps)))
        done, win = tr["done"].cpu().numpy() != 0, tr["winner"].cpu().numpy()
        first = win[done.argmax(0), np.arange(games)][done.any(0)]
        mine = 1 if guarded == 0 else -1
        wins, losses = wins + int((first == mine).sum()), losses + int((first == -mine).sum())
    return wins, losses


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cpu")
    ap.add_argument("--boards", type=int, default=128)
    ap.add_argument("--plies", type=int, default=16)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, gumbel in (("guarded (depth %d)" % a.depth, dict(considered=16, solve_depth=a.depth)), ("unguarded        ", dict(considered=16))):
        rows, kinds, share, loss = windows(a.device, gumbel, a.boards, a.plies, a.windows, a.steps)
        print("%s %d rows kept of %d plies; plies by how %s (%d = nat.HOW_PROVEN, %d = nat.HOW_GUMBEL); proven share of the guarded plies %.2f; "
              "last policy / value loss %.3f / %.3f" % (name, rows, a.boards * a.plies * a.windows, kinds, nat.HOW_PROVEN, nat.HOW_GUMBEL, share, *loss))
    w, l = arena(a.device, a.depth)
    print("arena, guarded Gumbel-16 against unguarded Gumbel-16 (the same untrained network, both colours): %d : %d" % (w, l))
