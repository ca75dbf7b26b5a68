#!/usr/bin/env python3
"""Stale search targets against reanalysed ones, from the same ring and the same seed.  Two generations of evaluator self-play go into
one ReplayBuffer: the first window is played by the untrained network, a trainer fits on it, and its network plays the second window.
The ring then holds visit counts of two different networks.  One GobbletTrainer fits on the ring as it stands (the stale targets); a
second one on a copy of the ring after ``buf.reanalyse(new_evaluator)`` -- every row's visits replaced in place by the visit counts of
the NEW network's search on the stored position (``gbl_reanalyse``, one launch; z stays the game's outcome).  Both networks are then
asked about held-out rows and the tablebase judges them, as examples/example_train_tablebase.py does: the share of rows whose value
has the right sign, and the share whose top prior keeps the game-theoretic result.
    python examples/example_reanalyse.py [device] [--inventory 2 2 0] [--boards N] [--plies T] [--steps S] [--iterations I]
Whether reanalysis helps a fit is printed, not claimed: it depends on the seed, the budget and how far apart the generations are."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gobblet_rl_amd as G  # noqa: E402
from example_train_tablebase import judge, window  # noqa: E402


def train_both(device, inventory=(2, 2, 0), boards=512, plies=32, steps=200, batch=1024, hidden=64, iterations=64, capacity=65536,
               held_out=4096, explore=16):
    """{"stale": ..., "reanalysed": ...}: per fit the held-out rows the table could label and the two shares; "reanalysed" also holds
    "mean_drift", the mean total variation between the stored and the fresh visit shares over the ring's rows (0 .. 1)."""
    tb = G.Tablebase(inventory, device)
    tb.build()
    first = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
    buf = G.ReplayBuffer(capacity, device)
    buf.append(*window(device, first.evaluator(), boards, plies, iterations, seed=1), tag=0)      # generation 0: the untrained network plays
    buf.fit(first, steps, batch=batch, symmetries="all")
    new = first.evaluator()
    buf.append(*window(device, new, boards, plies, iterations, seed=2), tag=1)                      # generation 1: its successor plays
    fresh = G.ReplayBuffer(capacity, device)
    fresh.append(*window(device, new, boards, plies, iterations, seed=1000), tag=0)
    rows = {k: v for k, v in fresh.batch(held_out, symmetries=None, seed=5).items() if k in ("observation", "action_mask", "visits", "z")}
    again = G.ReplayBuffer(capacity, device)
    again.load_state_dict(buf.state_dict())
    moved = again.reanalyse(new, iterations=iterations, explore=explore)["drift"]
    counted = moved >= 0
    mean_drift = float(moved[counted].float().mean()) / 1024.0 if bool(counted.any()) else 0.0
    out = {}
    for name, ring in (("stale", buf), ("reanalysed", again)):
        trainer = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
        ring.fit(trainer, steps, batch=batch, symmetries="all")
        count, value_sign, top_in_r = judge(tb, trainer.evaluator(), rows)
        out[name] = {"rows": count, "value_sign": value_sign, "top_prior_in_R": top_in_r}
    out["reanalysed"]["mean_drift"] = mean_drift
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cuda:0")
    ap.add_argument("--inventory", type=int, nargs=3, default=[2, 2, 0])
    ap.add_argument("--boards", type=int, default=512)
    ap.add_argument("--plies", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=64)
    a = ap.parse_args()
    res = train_both(a.device, tuple(a.inventory), a.boards, a.plies, a.steps, a.batch, iterations=a.iterations)
    print("the ring's targets moved by %.1f %% (mean total variation) under the new network's search" % (100 * res["reanalysed"]["mean_drift"]))
    for name, r in res.items():
        print("fit on %-10s targets: of %d held-out rows the value's sign is right on %.1f %%, the top prior keeps the result on %.1f %%"
              % (name, r["rows"], 100 * r["value_sign"], 100 * r["top_prior_in_R"]))
