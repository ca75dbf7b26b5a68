"""``TreeSearchGobbletPolicy`` -- a UCT tree search for N boards at once: one independent tree per board, ``iterations`` leaves of
``playouts`` masked-random games each (at most ``max_plies`` plies per game), the decision = the most visited root action.  Where
flat Monte-Carlo (``MonteCarloGobbletPolicy``) spends its playouts evenly over the root actions, the tree puts them where the
replies and counter-replies matter; the root visit distribution and value are the usual training targets.

The surface mirrors ``MonteCarloGobbletPolicy`` (``compute_actions`` / ``compute_actions_from_state`` / ``compute_action`` /
``compute_actions_rllib`` / ``forward`` / ``action_values``) and adds ``visit_distribution``.  One launch of ``gbl_tree_search``
per call (include/gobblet_hip.h): the search of call c draws from generator stream 3 keyed by (seed, global board, iteration,
playout, c), so two calls on the same boards search differently, and a shard of a batch (``env_base``) decides its boards exactly
as the whole batch would.  The search is integer-only: the kernel and the host flavour (``device="cpu"``) agree bit for bit.
"""
from __future__ import annotations

from typing import Any

import torch

from . import _native as nat
from ._policy_base import _TreeSearchPolicy


class TreeSearchGobbletPolicy(_TreeSearchPolicy):
    def __init__(self, iterations: int = 256, playouts: int = 16, max_plies: int = 64, explore: int = 16, seed: int = 0,
                 device="cuda:0", env_base: int = 0, **kwargs: Any) -> None:
        """iterations: leaves per decision (1 .. 1024); playouts: games per leaf (1 .. 256); max_plies: masked-random plies per game
        (0 .. 255) -- a game still open then counts as neither won nor lost; explore: weight of the exploration term in 1/256 of a
        full win (0 .. 1024; the default is the best of the sweep in profiles/r08/tree_policy.json); env_base: global index of
        board 0 of the batches this policy is handed (as ``BatchedGobblet``)."""
        for name, val, lo, hi in (("iterations", iterations, 1, 1024), ("playouts", playouts, 1, 256),
                                  ("max_plies", max_plies, 0, 255), ("explore", explore, 0, 1024)):
            if not lo <= int(val) <= hi:
                raise ValueError(f"{name} must be in [{lo}, {hi}]")
        self.iterations, self.playouts, self.max_plies, self.explore = int(iterations), int(playouts), int(max_plies), int(explore)
        self._games_per_visit = self.playouts  # (a leaf is `playouts` games)
        self.seed = int(seed or 0)
        self.env_base = int(env_base)
        self.device = nat.device(device)
        self._lib = nat.lib_for(self.device)  # ("cpu": the host flavour of the ABI, asked for -- never a fallback)
        self._calls = 0  # call index (keys the search's draws); +1 per call
        # outputs of the last call (tensors on the device): int32 (N, 54) visits / wins / losses of the root's children from the
        # mover's side, int32 (N,) nodes created and plies played, int32 (N,) the decision
        self.last_visits = self.last_wins = self.last_losses = self.last_nodes = self.last_plies = self.last_action = None

    def _run(self, state: torch.Tensor, to_move: torch.Tensor, mask) -> torch.Tensor:
        n = state.shape[0]
        visits = torch.empty((n, nat.ACTIONS), dtype=torch.int32, device=self.device)
        wins, losses = torch.empty_like(visits), torch.empty_like(visits)
        act = torch.empty(n, dtype=torch.int32, device=self.device)
        nodes, plies = torch.empty_like(act), torch.empty_like(act)
        with self._on_device():
            nat.check(self._lib.gbl_tree_search(state.data_ptr(), to_move.data_ptr(), nat.ptr(mask), self.iterations, self.playouts,
                                                self.max_plies, self.explore, self.seed, self.env_base, self._calls,
                                                visits.data_ptr(), wins.data_ptr(), losses.data_ptr(), act.data_ptr(),
                                                nodes.data_ptr(), plies.data_ptr(), n, self._stream()), "gbl_tree_search")
        self._calls += 1
        self.last_visits, self.last_wins, self.last_losses = visits, wins, losses
        self.last_nodes, self.last_plies, self.last_action = nodes, plies, act
        return act

