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

import contextlib
from typing import Any

import numpy as np
import torch

from . import _native as nat


class MonteCarloGobbletPolicy:
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
        self.device = torch.device(device)
        self._lib = nat.lib_for(self.device)  # ("cpu": the host flavour of the ABI, asked for -- never a fallback)
        self._calls = 0  # call index (keys the playouts' draws); +1 per call
        # outputs of the last call (tensors on the device): int32 (N, 54) wins / losses of the mover, int32 (N,) plies played
        self.last_wins = self.last_losses = self.last_plies = None
        self.last_action = None  # int32 (N,): the decision of action_values()' playouts

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

    def compute_actions_from_state(self, state: torch.Tensor, to_move: torch.Tensor, mask=None) -> torch.Tensor:
        """The decision from ``squares`` (N,27) + ``to_move`` (N,): int32 (N,), -1 where a board has no candidate."""
        return self._run(state, to_move, mask)

    def action_values(self, state: torch.Tensor, to_move: torch.Tensor, mask=None) -> torch.Tensor:
        """float32 (N, 54): (wins - losses) / playouts of every candidate action, -inf elsewhere (one call; the decision of the
        same playouts is left in ``last_action``)."""
        self.last_action = self._run(state, to_move, mask)
        vals = (self.last_wins - self.last_losses).to(torch.float32) / self.playouts
        n = vals.shape[0]
        legal = torch.empty((n, nat.ACTIONS), dtype=torch.int8, device=self.device)
        st = torch.as_tensor(state).to(device=self.device, dtype=torch.int8).reshape(n, nat.CELLS).contiguous()
        tm = torch.as_tensor(to_move).to(device=self.device, dtype=torch.int8).reshape(n).contiguous()
        with self._on_device():
            nat.check(self._lib.gbl_legal_mask(st.data_ptr(), tm.data_ptr(), legal.data_ptr(), n, self._stream()),
                      "gbl_legal_mask")
        cand = legal != 0
        if mask is not None:
            cand &= torch.as_tensor(mask).to(self.device).reshape(n, nat.ACTIONS) != 0
        return torch.where(cand, vals, torch.full_like(vals, float("-inf")))

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

