#!/usr/bin/env python3
"""Three fits from the same self-play, the same seed and the same start: uniform draws, draws by the tablebase's regret classes
(example_prioritized_replay.py's two), and the closed loop of prioritised replay -- every step draws by priority, weighs its rows by
their importance weights (``beta`` annealed from 0.4 to 1.0), and hands the trainer's own per-row loss back as the rows' next priority
(``fit(..., prioritized=True, beta=(0.4, 1.0), priority=dict(scale=, floor=, cap=))``: nine launches a step, nothing read by the host).
All three learn from the table's exact labels and are asked about held-out rows of another seed; the table judges the answers.
    python examples/example_per_fit.py [device] [--inventory 2 2 0] [--windows W] [--boards N] [--plies T] [--steps S]
The default inventory is small enough for device "cpu".  Whether any of it helps is not claimed: the program prints all three."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import example_prioritized_replay as P  # noqa: E402  (the judged windows and the regret table)
import example_train_tablebase as T  # noqa: E402  (the held-out verdict)
import gobblet_rl_amd as G  # noqa: E402

# priority = min(floor + int(1000 * (policy loss + value loss)), cap); a row nobody has drawn yet sits at the cap, as new rows usually do
PRIORITY = dict(scale=1000, floor=1, cap=10000)
FITS = ("uniform", "regret_table", "loss_driven")


def per_fit(device, inventory=(2, 2, 0), windows=2, boards=256, plies=24, steps=100, batch=512, hidden=64, iterations=32, capacity=32768,
            held_out=2048):
    """{fit: {"rows", "value_sign", "top_prior_in_R"}} for the three fits, and "rows" the rows collected."""
    tb = G.Tablebase(inventory, device)
    tb.build()
    start = G.GobbletTrainer(hidden=hidden, device=device, seed=0).evaluator()
    table = torch.tensor(P.WEIGHTS, dtype=torch.int32, device=device)
    buf = G.ReplayBuffer(capacity, device, prioritized=True)
    for g in range(windows):
        env, traj, _ = P.judged_window(device, start, tb, boards, plies, iterations, seed=1 + g)
        buf.append(env, traj, tag=g, priority=table[traj["regret"].long() + 1])
    fresh = G.ReplayBuffer(capacity, device)
    fresh.append(*T.window(device, start, boards, plies, iterations, seed=1000), tag=0)
    rows = {k: v for k, v in fresh.batch(held_out, symmetries=None, seed=5).items() if k in ("observation", "action_mask", "visits", "z")}
    out = {"rows": buf.size}
    for name in FITS:
        trainer = G.GobbletTrainer(hidden=hidden, device=device, seed=0)
        if name == "loss_driven":
            buf.set_all_priority(torch.full((buf.size,), PRIORITY["cap"], dtype=torch.int32, device=device))
            buf.fit(trainer, steps, batch=batch, symmetries="all", targets=tb, prioritized=True, beta=(0.4, 1.0), priority=PRIORITY)
        else:
            buf.fit(trainer, steps, batch=batch, symmetries="all", targets=tb, prioritized=name == "regret_table")
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
    res = per_fit(a.device, tuple(a.inventory), a.windows, a.boards, a.plies, a.steps, a.batch, iterations=a.iterations)
    print("%d rows" % res["rows"])
    for name in FITS:
        r = res[name]
        print("fit on %-12s draws: of %d held-out rows the value's sign is right on %.1f %%, the top prior keeps the result on %.1f %%"
              % (name, r["rows"], 100 * r["value_sign"], 100 * r["top_prior_in_R"]))
