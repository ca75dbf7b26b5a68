#!/usr/bin/env python3
"""The Gumbel root search in self-play, beside the PUCT search it stands in for at small budgets, from the same boards and the same
seed, on the host flavour by default.  A few windows of evaluator against evaluator (an untrained seeded network) go through
``outcome_targets`` into a ReplayBuffer and a short fit, twice: once with ``search=dict(iterations=16, gumbel=dict(considered=16))``
(``gbl_collect_search_gumbel``: Gumbel noise once per root, the 16 best actions by noise + logit, sequential halving, and the
completed-Q improved policy as the target -- every searched ply is a row), once with the PUCT search at 64 iterations
(``gbl_collect_search_eval``), one launch per window either way.  Printed per run: the rows the buffer kept per window, the network
evaluations (the sum of "nodes") per kept row, and the fit's last policy and value loss.
    python examples/example_gumbel.py [device] [--boards N] [--plies T] [--windows W] [--iterations I] [--considered M] [--steps S]
One seed, no claim: whether Gumbel windows train a better network per second of self-play is not shown here."""
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


def play(device, search, boards=256, plies=16, windows=4, steps=50, seed=1):
    """`windows` windows of `plies` plies with ``search`` (the evaluator is added here), appended and fitted.  Returns the per-window
    kept rows, the evaluations, the plies by `how` code and the fit's last (policy loss, value loss)."""
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    buf = G.ReplayBuffer(boards * plies * windows, device)
    search = dict(search, evaluator=seeded_evaluator(device))
    kept, evaluations, kinds = [], 0, {}
    for w in range(windows):
        tr = env.collect(plies, policies=("evaluator", "evaluator"), search=search)
        env.outcome_targets(tr)
        before = buf.total
        buf.append(env, tr, tag=w)
        kept.append(buf.total - before)
        evaluations += int(tr["nodes"].to(torch.int64).sum())
        for code, count in zip(*np.unique(tr["how"].cpu().numpy(), return_counts=True)):
            kinds[int(code)] = kinds.get(int(code), 0) + int(count)
    trainer = G.GobbletTrainer(64, device, seed=0)
    stats = buf.fit(trainer, steps, batch=512, symmetries=None)
    return kept, evaluations, kinds, (float(stats[-1, 0]), float(stats[-1, 1]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cpu")
    ap.add_argument("--boards", type=int, default=256)
    ap.add_argument("--plies", type=int, default=16)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=16)
    ap.add_argument("--considered", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    runs = (("gumbel %3d" % a.iterations, dict(iterations=a.iterations, gumbel=dict(considered=a.considered))),
            ("puct    64", dict(iterations=64, sample_plies=4)))
    for name, search in runs:
        kept, evaluations, kinds, loss = play(a.device, search, a.boards, a.plies, a.windows, a.steps)
        print("%s rows kept per window %s, %d evaluations, %.1f per kept row; plies by how %s (%d = nat.HOW_GUMBEL); last policy / value loss "
              "%.3f / %.3f" % (name, kept, evaluations, evaluations / max(sum(kept), 1), kinds, nat.HOW_GUMBEL, *loss))
