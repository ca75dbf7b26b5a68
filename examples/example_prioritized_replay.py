#!/usr/bin/env python3
"""Uniform against prioritised replay, from the same self-play and the same seed: example_train_tablebase.py's loop with the table as
a judge inside the self-play launch (``search=dict(tablebase=tb, judge=True)``).  ``Tablebase.judge`` gives every ply a regret class --
the played action kept the result, turned a win into a draw, a win into a loss, a draw into a loss, or the table has no verdict -- and the
rows go into one ``ReplayBuffer(prioritized=True)`` with a priority from a small weight table over those classes.  One GobbletTrainer
then fits on uniform draws, a second one on draws proportional to the priorities (``fit(..., prioritized=True)``), both on the table's
exact labels; both are asked about held-out rows of another seed and the table judges the answers.
    python examples/example_prioritized_replay.py [device] [--inventory 2 2 0] [--windows W] [--boards N] [--plies T] [--steps S]
A small inventory (the default here) also runs with device "cpu".  Whether prioritising helps is not claimed: the program prints both."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import example_train_tablebase as T  # noqa: E402  (the held-out verdict)
import gobblet_rl_amd as G  # noqa: E402

# priority per regret class, indexed by regret + 1: no verdict, kept, win -> draw, win -> loss, draw -> loss.  A thrown win is worth eight
# rows that kept the result; a row the table cannot label is still drawn now and then.  (All different: the report below tells the
# classes apart by their weight.)
WEIGHTS = (1, 2, 8, 16, 12)


def judged_window(device, ev, tb, boards, plies, iterations, seed):
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("evaluator", "evaluator"),
                       search=dict(evaluator=ev, iterations=iterations, sample_plies=4, noise=0.25, tablebase=tb, judge=True))
    env.outcome_targets(traj)
    counts = tb.judge(traj, boards)
    return env, traj, counts


def prioritized_replay(device, inventory=(2, 2, 0), windows=2, boards=256, plies=24, steps=100, batch=512, hidden=64, iterations=32,
                       capacity=32768, held_out=2048):
    """{"uniform": ..., "prioritized": ...}: per fit the held-out rows the table could label and the two shares of
    example_train_tablebase.py; "rows" the rows collected, "weight_by_class" the ring's weight per regret class."""
    tb = G.Tablebase(inventory, device)
    tb.build()
    start = G.GobbletTrainer(hidden=hidden, device=device, seed=0).evaluator()
    table = torch.tensor(WEIGHTS, dtype=torch.int32, device=device)
    buf = G.ReplayBuffer(capacity, device, prioritized=True)
    for g in range(windows):
        env, traj, _ = judged_window(device, start, tb, boards, plies, iterations, seed=1 + g)
        buf.append(env, traj, tag=g, priority=table[traj["regret"].long() + 1])
    fresh = G.ReplayBuffer(capacity, device)
    fresh.append(*T.window(device, start, boards, plies, iterations, seed=1000), tag=0)
    rows = {k: v for k, v in fresh.batch(held_out, symmetries=None, seed=5).items() if k in ("observation", "action_mask", "visits", "z")}
    live = buf.priority[:buf.size]
    out = {"rows": buf.size, "weight_by_class": {name: int(live[live == w].sum()) for name, w in
                                                 zip(("no_verdict",) + G.Tablebase.REGRET_CLASSES[:4], WEIGHTS)}}
    for name, prioritized in (("uniform", False), ("prioritized", True)):
        trainer = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
        buf.fit(trainer, steps, batch=batch, symmetries="all", targets=tb, prioritized=prioritized)
        count, value_sign, top_in_r = T.judge(tb, trainer.evaluator(), rows)
        out[name] = {"rows": count, "value_sign": value_sign, "top_prior_in_R": top_in_r}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cuda:0")
    ap.add_argument("--inventory", type=int, nargs=3, default=[2, 2, 0])
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--boards", type=int, default=256)
    ap.add_argument("--plies", type=int, default=24)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=32)
    a = ap.parse_args()
    res = prioritized_replay(a.device, tuple(a.inventory), a.windows, a.boards, a.plies, a.steps, a.batch, iterations=a.iterations)
    print("%d rows; weight by regret class: %s" % (res["rows"], res["weight_by_class"]))
    for name in ("uniform", "prioritized"):
        r = res[name]
        print("fit on %-11s draws: of %d held-out rows the value's sign is right on %.1f %%, the top prior keeps the result on %.1f %%"
              % (name, r["rows"], 100 * r["value_sign"], 100 * r["top_prior_in_R"]))
