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

import contextlib
from typing import Any

import numpy as np
import torch

from . import _native as nat


class TreeSearchGobbletPolicy:
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
        self.seed = int(seed or 0)
        self.env_base = int(env_base)
        self.device = torch.device(device)
        self._lib = nat.lib_for(self.device)  # ("cpu": the host flavour of the ABI, asked for -- never a fallback)
        self._calls = 0  # call index (keys the search's draws); +1 per call
        # outputs of the last call (tensors on the device): int32 (N, 54) visits / wins / losses of the root's children from the
        # mover's side, int32 (N,) nodes created and plies played, int32 (N,) the decision
        self.last_visits = self.last_wins = self.last_losses = self.last_nodes = self.last_plies = self.last_action = None

    def _stream(self):
        return nat.current_stream(self.device)

    def _on_device(self):
        """Launches go to the policy's device (on its current stream), whichever device is current."""
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    def _run(self, state: torch.Tensor, to_move: torch.Tensor, mask) -> torch.Tensor:
        state = torch.as_tensor(state).to(device=self.device, dtype=torch.int8).reshape(-1, nat.CELLS).contiguous()
        n = state.shape[0]
        to_move = torch.as_tensor(to_move).to(device=self.device, dtype=torch.int8).reshape(n).contiguous()
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=self.device, dtype=torch.int8).reshape(n, nat.ACTIONS).contiguous()
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

    def compute_actions_from_state(self, state: torch.Tensor, to_move: torch.Tensor, mask=None) -> torch.Tensor:
        """The decision from ``squares`` (N,27) + ``to_move`` (N,): int32 (N,), -1 where a board has no candidate."""
        return self._run(state, to_move, mask)

    def visit_distribution(self, state: torch.Tensor, to_move: torch.Tensor, mask=None) -> torch.Tensor:
        """float32 (N, 54): visits / iterations of every root action -- the policy target of a trainer; 0 for non-candidates (one
        call; the decision of the same search is left in ``last_action``)."""
        self._run(state, to_move, mask)
        return self.last_visits.to(torch.float32) / self.iterations

    def action_values(self, state: torch.Tensor, to_move: torch.Tensor, mask=None) -> torch.Tensor:
        """float32 (N, 54): (W - L) / (n * playouts) of every visited root action, -inf elsewhere (one call; the decision of the
        same search is left in ``last_action``)."""
        self._run(state, to_move, mask)
        seen = self.last_visits > 0
        games = (self.last_visits.clamp(min=1) * self.playouts).to(torch.float32)
        vals = (self.last_wins - self.last_losses).to(torch.float32) / games
        return torch.where(seen, vals, torch.full_like(vals, float("-inf")))

    def compute_actions(self, obs, mask=None) -> torch.Tensor:
        """obs: int8 (N,3,3,13); mask: int8 (N,54) or None (the legal mask of the board)."""
        obs = torch.as_tensor(obs).to(device=self.device, dtype=torch.int8).reshape(-1, 3, 3, 13).contiguous()
        n = obs.shape[0]
        state = torch.empty((n, nat.CELLS), dtype=torch.int8, device=self.device)
        who = torch.empty(n, dtype=torch.int8, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_decode_obs(obs.data_ptr(), state.data_ptr(), who.data_ptr(), n, self._stream()),
                      "gbl_decode_obs")
        return self._run(state, who, mask)

    # -- reference-shaped entry points (as GreedyGobbletPolicy) ----------------------------------------------
    def compute_action(self, obs, mask) -> np.ndarray:
        return np.array(int(self.compute_actions(np.asarray(obs)[None], np.asarray(mask)[None])[0]))

    def compute_actions_rllib(self, obs_batch):
        observations = np.asarray(obs_batch["observation"])
        observations = observations.reshape(observations.shape[0], 3, 3, -1)
        return list(self.compute_actions(observations, np.asarray(obs_batch["action_mask"])).cpu().numpy())

    def forward(self, batch, state=None, **kwargs):
        """Tianshou-adapter shape: ``batch.obs.obs`` / ``batch.obs.mask`` (or dict keys "obs" / "mask") -> {"act": int64 (N,)}."""
        ob = batch["obs"] if isinstance(batch, dict) else batch.obs
        obs = ob["obs"] if isinstance(ob, dict) else ob.obs
        mask = ob["mask"] if isinstance(ob, dict) else ob.mask
        act = self.compute_actions(obs, torch.as_tensor(mask).to(torch.int8))
        return {"act": act.to(torch.int64).cpu().numpy()}
