"""``MonteCarloGobbletPolicy`` -- a flat Monte-Carlo policy for N boards at once: for every candidate action it plays
``playouts`` masked-random games to the end (at most ``max_plies`` plies after the action) and picks the action with the
largest wins - losses.  Its strength grows with ``playouts``; the per-action counts are also the leaf values of a tree search.

The surface mirrors ``GreedyGobbletPolicy`` (``compute_actions`` / ``compute_actions_from_state`` / ``compute_action`` /
``compute_actions_rllib`` / ``forward``); ``action_values`` returns the values themselves.  One launch of
``gbl_playout_values`` per call (include/gobblet_hip.h): the playouts of call c draw from generator stream 2 keyed by
(seed, global board, action, playout, c), so two calls on the same boards play different games, and a shard of a batch
(``env_base``) decides its boards exactly as the whole batch would.
"""
from __future__ import annotations

from typing import Any

import torch

from . import _native as nat
from ._policy_base import _SearchPolicy


class MonteCarloGobbletPolicy(_SearchPolicy):
    def __init__(self, playouts: int = 64, max_plies: int = 64, seed: int = 0, device="cuda:0", env_base: int = 0,
                 **kwargs: Any) -> None:
        """playouts: games per candidate action (1 .. 4096); max_plies: masked-random plies per game after the action (0 .. 255)
        -- a game still open then counts as neither won nor lost.  env_base: global index of board 0 of the batches this policy
        is handed (as ``BatchedGobblet``)."""
        if not 1 <= int(playouts) <= 4096:
            raise ValueError("playouts must be in [1, 4096]")
        if not 0 <= int(max_plies) <= 255:
            raise ValueError("max_plies must be in [0, 255]")
        self.playouts, self.max_plies = int(playouts), int(max_plies)
        self.seed = int(seed or 0)
        self.env_base = int(env_base)
        self.device = nat.device(device)
        self._lib = nat.lib_for(self.device)  # ("cpu": the host flavour of the ABI, asked for -- never a fallback)
        self._calls = 0  # call index (keys the playouts' draws); +1 per call
        # outputs of the last call (tensors on the device): int32 (N, 54) wins / losses of the mover, int32 (N,) plies played
        self.last_wins = self.last_losses = self.last_plies = None
        self.last_action = None  # int32 (N,): the decision of action_values()' playouts

    def _run(self, state: torch.Tensor, to_move: torch.Tensor, mask) -> torch.Tensor:
        n = state.shape[0]
        wins = torch.empty((n, nat.ACTIONS), dtype=torch.int32, device=self.device)
        losses = torch.empty_like(wins)
        act = torch.empty(n, dtype=torch.int32, device=self.device)
        plies = torch.empty(n, dtype=torch.int32, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_playout_values(state.data_ptr(), to_move.data_ptr(), nat.ptr(mask), self.playouts,
                                                   self.max_plies, self.seed, self.env_base, self._calls, wins.data_ptr(),
                                                   losses.data_ptr(), act.data_ptr(), plies.data_ptr(), n, self._stream()),
                      "gbl_playout_values")
        self._calls += 1
        self.last_wins, self.last_losses, self.last_plies = wins, losses, plies
        return act

    def action_values(self, state: torch.Tensor, to_move: torch.Tensor, mask=None) -> torch.Tensor:
        """float32 (N, 54): (wins - losses) / playouts of every candidate action, -inf elsewhere (one call; the decision of the
        same playouts is left in ``last_action``)."""
        st, tm, m8 = self._inputs(state, to_move, mask)
        self.last_action = self._run(st, tm, m8)
        vals = (self.last_wins - self.last_losses).to(torch.float32) / self.playouts
        legal = torch.empty_like(vals, dtype=torch.int8)
        with self._on_device():
            nat.check(self._lib.gbl_legal_mask(st.data_ptr(), tm.data_ptr(), legal.data_ptr(), st.shape[0], self._stream()),
                      "gbl_legal_mask")
        cand = legal != 0
        if m8 is not None:
            cand &= m8 != 0
        return torch.where(cand, vals, torch.full_like(vals, float("-inf")))
