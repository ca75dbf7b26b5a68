#!/usr/bin/env python3
"""Search targets against exact targets, from the same self-play and the same seed: a few windows of evaluator self-play go into one
ReplayBuffer; one GobbletTrainer fits on what the search left there (visit counts, the outcome of the game a row belonged to), a second
one on the tablebase's labels for the very same draws (``fit(..., targets=tb)``: every action that keeps the true result, the true sign).
Both networks are then asked about held-out rows -- a window of another seed -- and the table judges them: the share of rows whose
value has the right sign, and the share whose top prior keeps the game-theoretic result.
    python examples/example_train_tablebase.py [device] [--inventory 2 2 2] [--windows W] [--boards N] [--plies T] [--steps S]
                                                [--table-play P]
``--table-play P`` (P > 0) adds a third network, fit on windows the table played against itself inside the launch
(``collect(policies=("tablebase", "tablebase"))``, the first P plies of every game drawn among the moves that keep the result): perfect
games that carry their exact targets as they are collected, instead of search games relabelled afterwards.
The full inventory's table takes 2.9 GB on the device and about half a second to build there; a smaller inventory (``--inventory 2 2 0``,
which also runs with device "cpu") labels only the rows whose boards hold no piece it lacks -- the others count for nothing."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402


def window(device, ev, boards, plies, iterations, seed):
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=iterations, sample_plies=4, noise=0.25))
    env.outcome_targets(traj)
    return env, traj


def table_window(device, tb, boards, plies, sample_plies, seed):
    """A window of table-against-table play: the visits rows are the table's labels already, the games' outcomes the true results."""
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("tablebase", "tablebase"), search=dict(tablebase=tb, tb_mode="result", sample_plies=sample_plies))
    env.outcome_targets(traj)
    return env, traj


def judge(tb, ev, rows):
    """The table's verdict on the evaluator's answers for the labelled rows of a batch dict: (rows, value-sign share, top-prior-in-R share)."""
    n = rows["z"].shape[0]
    truth = tb.targets({k: v.clone() for k, v in rows.items()}, mode="result")     # visits > 0 is R, z the true sign
    state = torch.empty((n, nat.CELLS), dtype=torch.int8, device=tb.device)
    who = torch.empty(n, dtype=torch.int8, device=tb.device)
    with tb._on_device():
        nat.check(tb._lib.gbl_decode_obs(rows["observation"].data_ptr(), state.data_ptr(), who.data_ptr(), n, tb._stream()), "gbl_decode_obs")
    priors, value, _ = ev.evaluate_raw(state, who, rows["action_mask"])
    labelled = truth["z"] != nat.Z_OPEN
    count = int(labelled.sum())
    if count == 0:
        return 0, 0.0, 0.0
    sign_right = (torch.sign(value) == truth["z"].to(torch.int32)) & labelled
    top = priors.to(torch.int32).argmax(1, keepdim=True)
    keeps = (truth["visits"].gather(1, top).reshape(-1) > 0) & labelled
    return count, float(sign_right.sum()) / count, float(keeps.sum()) / count


def train_both(device, inventory=(2, 2, 2), windows=3, boards=512, plies=32, steps=200, batch=1024, hidden=64, iterations=64, capacity=65536,
               held_out=4096, table_play=0):
    """{"search": ..., "exact": ...}: per network the held-out rows the table could label and the two shares; with table_play > 0
    also "table": a network fit on table-against-table windows whose first `table_play` plies per game are sampled."""
    tb = G.Tablebase(inventory, device)
    tb.build()
    start = G.GobbletTrainer(hidden=hidden, device=device, seed=0).evaluator()
    buf = G.ReplayBuffer(capacity, device)
    for g in range(windows):
        buf.append(*window(device, start, boards, plies, iterations, seed=1 + g), tag=g)
    fresh = G.ReplayBuffer(capacity, device)
    fresh.append(*window(device, start, boards, plies, iterations, seed=1000), tag=0)
    rows = {k: v for k, v in fresh.batch(held_out, symmetries=None, seed=5).items() if k in ("observation", "action_mask", "visits", "z")}
    out = {}
    for name, targets in (("search", None), ("exact", tb)):
        trainer = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
        buf.fit(trainer, steps, batch=batch, symmetries="all", targets=targets)
        count, value_sign, top_in_r = judge(tb, trainer.evaluator(), rows)
        out[name] = {"rows": count, "value_sign": value_sign, "top_prior_in_R": top_in_r}
    if table_play > 0:
        games = G.ReplayBuffer(capacity, device)
        for g in range(windows):
            games.append(*table_window(device, tb, boards, plies, table_play, seed=1 + g), tag=g)
        trainer = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
        games.fit(trainer, steps, batch=batch, symmetries="all")
        count, value_sign, top_in_r = judge(tb, trainer.evaluator(), rows)
        out["table"] = {"rows": count, "value_sign": value_sign, "top_prior_in_R": top_in_r}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cuda:0")
    ap.add_argument("--inventory", type=int, nargs=3, default=[2, 2, 2])
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--boards", type=int, default=512)
    ap.add_argument("--plies", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--table-play", type=int, default=0, metavar="P")
    a = ap.parse_args()
    res = train_both(a.device, tuple(a.inventory), a.windows, a.boards, a.plies, a.steps, a.batch, iterations=a.iterations,
                     table_play=a.table_play)
    for name, r in res.items():
        print("fit on %-6s targets: of %d held-out rows the value's sign is right on %.1f %%, the top prior keeps the result on %.1f %%"
              % (name, r["rows"], 100 * r["value_sign"], 100 * r["top_prior_in_R"]))
