#!/usr/bin/env python3
"""A Gumbel self-play ring refreshed by a newer network with the Gumbel root search.  The untrained network plays a window by the
Gumbel rule at 16 iterations (``collect(search=dict(gumbel=...))``: every searched ply is a dense target row, bytes 1 .. 255 on every
candidate), a trainer fits on the ring, and its network then refreshes the ring in place with ``buf.reanalyse(new, iterations=16,
gumbel=...)`` -- one launch of ``gbl_reanalyse_gumbel``: every live row's bytes become the NEW network's completed-Q policy on the
stored position, the same kind of row as before, so the drift measures how far the network has moved and not the difference between
two search rules.  z stays the game's outcome.
    python examples/example_reanalyse_gumbel.py [device] [--boards N] [--plies T] [--steps S] [--iterations I] [--considered M]
Prints the rows refreshed per network evaluation the budget allows (a row costs at most iterations + 1 evaluations) and the histogram of
the rows' drift.  Whether the refreshed targets train a better network is not measured here."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gobblet_rl_amd as G  # noqa: E402

BINS = 8  # the drift histogram's bins over 0 .. 1024


def refresh(device, boards=512, plies=32, steps=100, batch=1024, hidden=64, iterations=16, considered=16, capacity=65536, explore=16, seed=1):
    """{"rows", "evaluations", "rows_per_evaluation", "mean_drift" (0 .. 1), "drift_histogram" (BINS counts), "moved" (rows whose bytes
    changed)}: one Gumbel window by the untrained network, `steps` Adam steps on it, then the refresh by the fitted network."""
    rule = dict(considered=considered, noise=True)
    trainer = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=trainer.evaluator(), iterations=iterations,
                                                                               explore=explore, gumbel=rule))
    env.outcome_targets(traj)
    buf = G.ReplayBuffer(capacity, device)
    buf.append(env, traj, tag=0)
    buf.fit(trainer, steps, batch=min(batch, max(buf.size, 1)), symmetries="all")
    before = buf.visits[:buf.size].clone()
    out = buf.reanalyse(trainer.evaluator(), iterations=iterations, explore=explore, gumbel=rule, seed=seed, call=1)
    drift = out["drift"]
    counted = drift >= 0
    rows = int(counted.sum())
    evaluations = rows * (iterations + 1)
    hist = torch.bincount((drift[counted].clamp(max=1023) * BINS // 1024).to(torch.int64), minlength=BINS).tolist() if rows else [0] * BINS
    return {"rows": rows, "evaluations": evaluations, "rows_per_evaluation": rows / evaluations if evaluations else 0.0,
            "mean_drift": float(drift[counted].float().mean()) / 1024.0 if rows else 0.0, "drift_histogram": hist,
            "moved": int((buf.visits[:buf.size] != before).any(1).sum())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cuda:0")
    ap.add_argument("--boards", type=int, default=512)
    ap.add_argument("--plies", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=16)
    ap.add_argument("--considered", type=int, default=16)
    a = ap.parse_args()
    res = refresh(a.device, a.boards, a.plies, a.steps, a.batch, iterations=a.iterations, considered=a.considered)
    print("%d rows refreshed with at most %d evaluations: %.4f rows per evaluation; %d rows changed"
          % (res["rows"], res["evaluations"], res["rows_per_evaluation"], res["moved"]))
    print("mean drift %.1f %% (total variation between the stored and the fresh target rows); histogram over %d bins of 0 .. 100 %%: %s"
          % (100 * res["mean_drift"], BINS, res["drift_histogram"]))
