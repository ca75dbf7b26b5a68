#!/usr/bin/env python3
"""The loop closed end to end: tree-vs-tree self-play -> (obs, pi, z) targets -> a 117-H-55 MLP fitted in torch -> the integer
evaluator -> the evaluator-guided search against the playout search at equal iterations; with --generations G > 1 the loop goes
round: generation k collects with generation k - 1's evaluator on both sides INSIDE one launch (gbl_collect_search_eval), fits a
new network and plays it against the old one, one launch per colour:
    python examples/example_train_evaluator.py [device] [--boards N] [--plies T] [--steps S] [--hidden H] [--games G] [--generations G] [--noise X]
--augment square|all draws every Adam step's batch on the device under random board symmetries (BatchedGobblet.training_batch) and
fits there; the default (none) keeps the whole window on the host as before.  --fit device (with --augment) runs every Adam step on
the device too: BatchedGobblet.fit with a GobbletTrainer, two launches of gbl_train_step per step instead of torch's few dozen, and the
same bits from the same seed on every run; the default (torch) keeps the recorded runs reproducible."""
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
    return targets_of(traj, boards, plies)


def targets_of(traj, boards, plies):
    """(obs, pi, z) of the plies of finished games of a collected window with search outputs and outcome targets."""
    obs = traj["observation"][:-1].reshape(plies - 1, boards, 117)   # what the mover of ply t saw is slot t - 1
    visits, z = traj["visits"][1:].float(), traj["z"][1:]
    keep = (z != G._native.Z_OPEN) & (traj["done"][:-1] == 0) & (visits.sum(-1) > 0)  # (after a finished game slot t - 1 is a fresh board)
    pi = visits / visits.sum(-1, keepdim=True).clamp(min=1)
    return obs[keep].float().cpu(), pi[keep].cpu(), z[keep].float().cpu()


def collect_targets_with(ev, device, boards, plies, iterations, seed=0, solve_depth=0, noise=0.0):
    """collect_targets with the evaluator-guided search of `ev` on both sides, the first four plies of every game drawn in proportion
    to the visits: one launch for the whole window.  solve_depth > 0: the exact solver in front of every search (a proven win is
    taken, a proven loss avoided, and such a ply's policy target is one-hot).  noise > 0: that share of a random row is mixed into
    the root's priors of every search, so that the search also looks at what the network rates low (the arena never does this)."""
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("evaluator", "evaluator"),
                       search=dict(evaluator=ev, iterations=iterations, sample_plies=4, solve_depth=solve_depth, noise=noise))
    env.outcome_targets(traj)
    return targets_of(traj, boards, plies)


def arena_in_one_launch(new, old, device, games, plies, iterations, seed=7):
    """`new` against `old`, half the boards' games with either colour, each half ONE launch with auto-reset: every board plays game
    after game for `plies` plies and the wins are read from the counters.  (new wins, old wins, games finished)."""
    wins, losses, finished = 0, 0, 0
    for nets in ((new, old), (old, new)):
        env = G.BatchedGobblet(max(games // 2, 1), device, auto_reset=True, seed=seed)
        env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=nets, iterations=iterations), count=True, refresh=False)
        c = env.counters  # (plies, games finished, player_1 wins, player_2 wins)
        w1, w2 = int(c[2]), int(c[3])
        wins, losses, finished = wins + (w1 if nets[0] is new else w2), losses + (w2 if nets[0] is new else w1), finished + int(c[1])
    return wins, losses, finished


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


def fit_augmented(env, traj, hidden, steps, augment, seed=0):
    """fit() with every step's 1 024 rows drawn by env.training_batch(call=step) -- plies of finished games under random symmetries
    ("square": the 8 of the square, "all": the 512) -- on the device the window lies on; nothing of the window crosses to the host."""
    torch.manual_seed(seed)
    dev = env.device
    l1, l2 = torch.nn.Linear(117, hidden).to(dev), torch.nn.Linear(hidden, 55).to(dev)
    opt = torch.optim.Adam(list(l1.parameters()) + list(l2.parameters()), lr=2e-3, weight_decay=1e-4)
    loss, batch = torch.zeros(()), None
    for step in range(steps):
        batch = env.training_batch(traj, 1024, symmetries=augment, call=step, out=batch)
        drawn = (batch["index"][:, 0] >= 0).float()  # (a sample that found no finished ply in its 16 attempts counts for nothing)
        obs, visits, z = batch["observation"].float(), batch["visits"].float(), batch["z"].float() * drawn
        pi = visits / visits.sum(-1, keepdim=True).clamp(min=1)
        out = l2(torch.relu(l1(obs)))
        per = -(pi * torch.log_softmax(out[:, :54], 1)).sum(1) + (out[:, 54].clamp(-1, 1) - z) ** 2 + 1e-2 * out[:, 54] ** 2
        loss = (per * drawn).sum() / drawn.sum().clamp(min=1)
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        wide = env.training_batch(traj, 8192, symmetries=augment, call=steps)
        hmax = float(torch.relu(l1(wide["observation"].float())).max())
    return (l1.weight.detach().T, l1.bias.detach(), l2.weight.detach().T, l2.bias.detach()), hmax, float(loss.detach())


def fit_on_device(env, traj, hidden, steps, augment, seed=0):
    """fit_augmented with the whole step on the device: the batch draw and gbl_train_step, nothing of the fit in torch."""
    trainer = G.GobbletTrainer(hidden=hidden, device=env.device, seed=seed)
    stats = env.fit(traj, trainer, steps, batch=1024, symmetries=augment)
    return trainer.evaluator(), float(stats[-1, 0] + stats[-1, 1])


def arena(first, second, n, device, seed=7, max_plies=64):
    """n games in lockstep, `first` as player_1 (finished games stay frozen): (player_1 wins, player_2 wins)."""
    env = G.BatchedGobblet(n, device, auto_reset=False, seed=seed)
    for t in range(max_plies):
        if bool(env.done.all()):
            break
        a = (first if t % 2 == 0 else second).compute_actions_from_state(env.squares, env.to_move, env.action_mask)
        env.step(torch.where(env.done != 0, torch.zeros_like(a), a))
    return int((env.winner == 1).sum()), int((env.winner == -1).sum())


def train_evaluator(device, boards=512, plies=48, steps=400, hidden=64, collect_iterations=64, augment="none", fit_with="torch"):
    if augment != "none":
        env = G.BatchedGobblet(boards, device, auto_reset=True, seed=0, track_turn=True)
        traj = env.collect(plies, policies=("tree", "tree"), search=dict(iterations=collect_iterations, playouts=8, max_plies=64, explore=16,
                                                                         sample_plies=4))
        env.outcome_targets(traj)
        kept = int(((traj["z"][1:] != G._native.Z_OPEN) & (traj["done"][:-1] == 0) & (traj["visits"][1:].sum(-1, dtype=torch.int32) > 0)).sum())
        if fit_with == "device":
            ev, loss = fit_on_device(env, traj, hidden, steps, augment)
            return ev, kept, loss
        weights, hmax, loss = fit_augmented(env, traj, hidden, steps, augment)
        return G.GobbletEvaluator.from_float(*weights, hidden_max=hmax, device=device), kept, loss
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
    ap.add_argument("--generations", type=int, default=1)
    ap.add_argument("--selfplay-iterations", type=int, default=64, help="iterations of the evaluator search in generations >= 2")
    ap.add_argument("--solve-depth", type=int, default=0,
                    help="guard the self-play of generations >= 2 with the exact solver at this depth (0: none)")
    ap.add_argument("--noise", type=float, default=0.0,
                    help="share in [0, 1] of root exploration noise in the self-play of generations >= 2 (0: none; never in the arena)")
    ap.add_argument("--augment", choices=("none", "square", "all"), default="none",
                    help="draw every step's batch on the device under random board symmetries (generation 1)")
    ap.add_argument("--fit", choices=("torch", "device"), default="torch",
                    help="device: every Adam step of generation 1 is gbl_train_step (needs --augment square or all)")
    a = ap.parse_args()
    if a.fit == "device" and a.augment == "none":
        ap.error("--fit device draws its batches on the device: pass --augment square or all")
    ev, samples, loss = train_evaluator(a.device, a.boards, a.plies, a.steps, a.hidden, augment=a.augment, fit_with=a.fit)
    print("trained on", samples, "plies; final loss", round(loss, 3), "; scales", ev.scales, "shifts", (ev.shift1, ev.shift_p, ev.shift_v))
    w, l, d = score(ev, a.device, a.iterations, a.games)
    print("evaluator search vs playout search at %d iterations: %d wins, %d losses, %d unfinished of %d games" % (a.iterations, w, l, d, w + l + d))
    for gen in range(2, a.generations + 1):
        obs, pi, z = collect_targets_with(ev, a.device, a.boards, a.plies, a.selfplay_iterations, seed=gen, solve_depth=a.solve_depth,
                                          noise=a.noise)
        weights, hmax, loss = fit(obs, pi, z, a.hidden, a.steps, seed=gen)
        new = G.GobbletEvaluator.from_float(*weights, hidden_max=hmax, device=a.device)
        w, l, n = arena_in_one_launch(new, ev, a.device, a.games, a.plies, a.selfplay_iterations)
        print("generation %d: trained on %d plies of generation %d's self-play, final loss %.3f; arena against generation %d at %d "
              "iterations: %d wins, %d losses of %d finished games" % (gen, len(obs), gen - 1, loss, gen - 1, a.selfplay_iterations, w, l, n))
        ev = new
