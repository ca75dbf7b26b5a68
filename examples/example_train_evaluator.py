#!/usr/bin/env python3
"""The loop closed end to end: tree-vs-tree self-play -> (obs, pi, z) targets -> a 117-H-55 MLP fitted in torch -> the integer
evaluator -> the evaluator-guided search against the playout search at equal iterations:
    python examples/example_train_evaluator.py [device] [--boards N] [--plies T] [--steps S] [--hidden H] [--games G]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gobblet_rl_amd as G  # noqa: E402


def collect_targets(device, boards, plies, iterations, seed=0):
    """(obs float (M, 117), pi float (M, 54), z float (M,)) of the plies of finished games of tree-vs-tree self-play."""
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    search = dict(iterations=iterations, playouts=8, max_plies=64, explore=16, sample_plies=4)
    traj = env.collect(plies, policies=("tree", "tree"), search=search)
    env.outcome_targets(traj)
    obs = traj["observation"][:-1].reshape(plies - 1, boards, 117)   # what the mover of ply t saw is slot t - 1
    visits, z = traj["visits"][1:].float(), traj["z"][1:]
    keep = (z != G._native.Z_OPEN) & (traj["done"][:-1] == 0) & (visits.sum(-1) > 0)  # (after a finished game slot t - 1 is a fresh board)
    pi = visits / visits.sum(-1, keepdim=True).clamp(min=1)
    return obs[keep].float().cpu(), pi[keep].cpu(), z[keep].float().cpu()


def fit(obs, pi, z, hidden, steps, seed=0):
    """A bounded number of Adam steps on cross-entropy(pi) + MSE(clip(value), z); returns the float weights from_float takes."""
    torch.manual_seed(seed)
    l1, l2 = torch.nn.Linear(117, hidden), torch.nn.Linear(hidden, 55)
    opt = torch.optim.Adam(list(l1.parameters()) + list(l2.parameters()), lr=2e-3, weight_decay=1e-4)
    loss = torch.zeros(())
    for step in range(steps):
        idx = torch.randint(0, len(obs), (min(1024, len(obs)),))
        out = l2(torch.relu(l1(obs[idx])))
        loss = -(pi[idx] * torch.log_softmax(out[:, :54], 1)).sum(1).mean() + ((out[:, 54].clamp(-1, 1) - z[idx]) ** 2).mean() \
            + 1e-2 * (out[:, 54] ** 2).mean()  # (keeps the value column small where the clip has no gradient)
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        hmax = float(torch.relu(l1(obs)).max())
    return (l1.weight.detach().T, l1.bias.detach(), l2.weight.detach().T, l2.bias.detach()), hmax, float(loss.detach())


def arena(first, second, n, device, seed=7, max_plies=64):
    """n games in lockstep, `first` as player_1 (finished games stay frozen): (player_1 wins, player_2 wins)."""
    env = G.BatchedGobblet(n, device, auto_reset=False, seed=seed)
    for t in range(max_plies):
        if bool(env.done.all()):
            break
        a = (first if t % 2 == 0 else second).compute_actions_from_state(env.squares, env.to_move, env.action_mask)
        env.step(torch.where(env.done != 0, torch.zeros_like(a), a))
    return int((env.winner == 1).sum()), int((env.winner == -1).sum())


def train_evaluator(device, boards=512, plies=48, steps=400, hidden=64, collect_iterations=64):
    obs, pi, z = collect_targets(device, boards, plies, collect_iterations)
    weights, hmax, loss = fit(obs, pi, z, hidden, steps)
    return G.GobbletEvaluator.from_float(*weights, hidden_max=hmax, device=device), len(obs), loss


def score(ev, device, iterations, games, explore=None):
    """Evaluator search against the playout search at equal iterations, both colours: (wins, losses, draws) of the evaluator."""
    kw = {} if explore is None else {"explore": explore}
    mine = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=iterations, device=device, **kw)
    theirs = G.TreeSearchGobbletPolicy(iterations=iterations, playouts=16, seed=0, device=device)
    w1, l1 = arena(mine, theirs, games // 2, device)
    l2, w2 = arena(theirs, mine, games // 2, device)
    return w1 + w2, l1 + l2, 2 * (games // 2) - w1 - w2 - l1 - l2


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("device", nargs="?", default="cuda:0")
    ap.add_argument("--boards", type=int, default=512)
    ap.add_argument("--plies", type=int, default=48)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--games", type=int, default=128)
    a = ap.parse_args()
    ev, samples, loss = train_evaluator(a.device, a.boards, a.plies, a.steps, a.hidden)
    print("trained on", samples, "plies; final loss", round(loss, 3), "; scales", ev.scales, "shifts", (ev.shift1, ev.shift_p, ev.shift_v))
    w, l, d = score(ev, a.device, a.iterations, a.games)
    print("evaluator search vs playout search at %d iterations: %d wins, %d losses, %d unfinished of %d games" % (a.iterations, w, l, d, w + l + d))
