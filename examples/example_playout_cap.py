#!/usr/bin/env python3
"""Playout-cap randomisation of evaluator self-play, with and without it, from the same boards and the same seed, on the host
flavour by default.  A few windows of evaluator against evaluator (an untrained seeded network, the solver's guard on player_1) go
through ``outcome_targets`` into a ReplayBuffer twice: once with every ply searched in full, once with
``search=dict(cap=dict(fast_iterations=16, full=0.25))`` -- a quarter of the plies searched in full and recorded, the rest played from
16 iterations without noise and not recorded (``gbl_collect_search_cap``, one launch per window either way).  Printed per run: the
rows the buffer kept per window, the network evaluations (the sum of "nodes") per kept row, and the plies by kind per side.
    python examples/example_playout_cap.py [device] [--boards N] [--plies T] [--windows W] [--iterations I] [--fast F] [--full P]
One seed, no claim: whether capped self-play trains a better network per second of self-play is not shown here."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402


def seeded_evaluator(device, hidden=64, seed=0):
    rng = np.random.default_rng(seed)
    return G.GobbletEvaluator(rng.integers(-128, 128, (117, hidden), dtype=np.int8), rng.integers(-300, 300, hidden),
                              rng.integers(-128, 128, (hidden // 4, 56, 4), dtype=np.int8), rng.integers(-65536, 65536, 56), 1, 9, 9,
                              device=device)


def play(device, cap, boards=256, plies=16, windows=4, iterations=64, seed=1):
    """`windows` windows of `plies` plies; cap: None or the dict ``collect`` takes.  Returns the per-window kept rows, the evaluations,
    and per side the plies that were full / fast / proven."""
    ev = seeded_evaluator(device)
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    buf = G.ReplayBuffer(boards * plies * windows, device)
    search = dict(evaluator=ev, iterations=iterations, sample_plies=4, noise=0.25, solve_depth=(3, 0))
    if cap is not None:
        search["cap"] = cap
    kept, evaluations, kinds = [], 0, np.zeros((2, 3), np.int64)
    for w in range(windows):
        tr = env.collect(plies, policies=("evaluator", "evaluator"), search=search)
        env.outcome_targets(tr)
        before = buf.total
        buf.append(env, tr, tag=w)
        kept.append(buf.total - before)
        evaluations += int(tr["nodes"].to(torch.int64).sum())
        how, mover = tr["how"].cpu().numpy(), tr["mover"].cpu().numpy()
        for m in (0, 1):
            mine = how[mover == m]
            kinds[m] += (np.isin(mine, (nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED)).sum(), (mine >= nat.HOW_FAST).sum(),
                         (mine == nat.HOW_PROVEN).sum())
    return kept, evaluations, kinds


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cpu")
    ap.add_argument("--boards", type=int, default=256)
    ap.add_argument("--plies", type=int, default=16)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--fast", type=int, default=16)
    ap.add_argument("--full", type=float, default=0.25)
    a = ap.parse_args()
    for name, cap in (("uncapped", None), ("capped  ", dict(fast_iterations=a.fast, full=a.full))):
        kept, evaluations, kinds = play(a.device, cap, a.boards, a.plies, a.windows, a.iterations)
        print("%s rows kept per window %s, %d evaluations, %.1f per kept row" % (name, kept, evaluations, evaluations / max(sum(kept), 1)))
        for m in (0, 1):
            print("         player_%d: %d full, %d fast, %d proven plies" % (m + 1, *kinds[m]))
