#!/usr/bin/env python3
"""Self-play with the tree search inside the launch, and the (observation, policy target, value target) tuples of an
AlphaZero-style trainer:  python examples/example_selfplay_search.py [cpu]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gobblet_rl_amd as G  # noqa: E402

device = sys.argv[1] if len(sys.argv) > 1 else "cuda:0"
env = G.BatchedGobblet(256, device, auto_reset=True, seed=0, track_turn=True)
search = dict(iterations=64, playouts=8, max_plies=64, explore=16, sample_plies=4)  # the first 4 plies of a game: drawn by visits
traj = env.collect(32, policies=("tree", "tree"), search=search)   # 32 plies of every board in ONE launch, every search kept
env.outcome_targets(traj)                                          # + "z" (the game's result for the mover) and "plies_left"

# the position a search looked at is the observation the ply BEFORE it left behind: pair ply t's search with slot t - 1
obs = traj["observation"][:-1]                                     # (31, N, 3, 3, 13): what the mover of ply t saw
pi = traj["visits"][1:].float() / traj["visits"][1:].sum(-1, keepdim=True).clamp(min=1)  # (31, N, 54): the policy target
z = traj["z"][1:]                                                  # (31, N): +1 / -1 for that mover, -128 = game still open
keep = z != G._native.Z_OPEN
print("plies collected:", int(keep.numel()), "with a finished game:", int(keep.sum()), "games finished:", int(traj["done"].sum()))
t, b = (int(x) for x in torch.nonzero(keep)[0])
print("one (obs, pi, z) tuple: obs", tuple(obs[t, b].shape), "own pieces on", int(obs[t, b, :, :, :6].sum()), "squares;",
      "pi top action", int(pi[t, b].argmax()), "with", round(float(pi[t, b].max()), 3), "; z", int(z[t, b]))
