#!/usr/bin/env python3
"""A Gumbel learner against the exact table, judged ply by ply, in one launch per window (``gbl_collect_gumbel_tb``), on the host
flavour by default.  ``search=dict(iterations=16, gumbel=dict(considered=16, tablebase=tb, judge=True))``: the "evaluator" side plays
the 16-iteration Gumbel search ("how" = ``nat.HOW_GUMBEL``, the completed-Q row as the target), the "tablebase" side plays from a small
complete table ("how" = ``nat.HOW_TABLE`` / ``nat.HOW_TABLE_SAMPLED``; on a board the table does not hold it moves at random), and the
table's verdict of EVERY ply lands beside the trajectory.  ``Tablebase.judge`` turns the verdicts into the census per side -- how often
a side kept the result and how often it threw a win or a draw away -- and into "regret" per ply, which drives the priorities of a
prioritised ReplayBuffer: a ply that threw a result away is drawn more often.  A short fit follows.
    python examples/example_gumbel_tb.py [device] [--boards N] [--plies T] [--windows W] [--inventory a,b,c] [--steps S]
One seed, no claim beyond the printed lines."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
from example_gumbel import seeded_evaluator  # noqa: E402

# the priority of a row by its regret + 1: no verdict, kept, a win became a draw, a win became a loss, a draw became a loss
WEIGHTS = (1, 1, 4, 8, 8)


def main(device, boards, plies, windows, inventory, steps, seed=1):
    tb = G.Tablebase(inventory, device)
    tb.build()
    assert tb.complete
    print("the %s table: %d positions, complete after %d sweeps" % (inventory, tb.positions, tb.sweeps))
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    buf = G.ReplayBuffer(boards * plies * windows, device, prioritized=True)
    weights = torch.tensor(WEIGHTS, dtype=torch.int32, device=device)
    search = dict(evaluator=seeded_evaluator(device), iterations=16, sample_plies=2,
                  gumbel=dict(considered=16, tablebase=tb, tb_mode="result", tb_count=1, judge=True))
    total = {}
    for w in range(windows):
        # the learner takes either colour in turn
        policies = ("evaluator", "tablebase") if w % 2 == 0 else ("tablebase", "evaluator")
        traj = env.collect(plies, policies=policies, search=search)
        census = tb.judge(traj)
        learner = "player_1" if w % 2 == 0 else "player_2"
        for side, counts in census.items():
            who = "Gumbel-16" if side == learner else "table    "
            print("window %d  %s (%s): %s" % (w, who, side, counts))
            for k, v in counts.items():
                total[(who, k)] = total.get((who, k), 0) + v
        env.outcome_targets(traj)
        buf.append(env, traj, tag=w, priority=weights[traj["regret"].long() + 1])
    for who in ("Gumbel-16", "table    "):
        judged = sum(v for (w_, k), v in total.items() if w_ == who and k != "no_verdict")
        lost = sum(v for (w_, k), v in total.items() if w_ == who and k not in ("kept", "no_verdict"))
        print("%s threw a result away on %d of %d judged plies" % (who, lost, judged))
    print("%d rows kept of %d plies (the valid cells with how %d, %d or %d); priority sum %d"
          % (buf.total, boards * plies * windows, nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED, nat.HOW_GUMBEL, int(buf.priority[:buf.total].sum())))
    if buf.total:
        stats = buf.fit(G.GobbletTrainer(64, device, seed=0), steps, batch=256, symmetries=None, prioritized=True, beta=0.5)
        print("last policy / value loss of %d prioritised steps: %.3f / %.3f" % (steps, float(stats[-1, 0]), float(stats[-1, 1])))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cpu")
    ap.add_argument("--boards", type=int, default=128)
    ap.add_argument("--plies", type=int, default=16)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--inventory", default="2,2,0")
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    torch.manual_seed(0)
    main(a.device, a.boards, a.plies, a.windows, tuple(int(x) for x in a.inventory.split(",")), a.steps)
