"""What the policy classes share (private: the public names are the policies themselves).

``_ReferenceAdapters``: the three reference-shaped entry points over a class's own batched ``compute_actions(obs, mask)``.
``_OnDevice``: the stream, the device context and the (state, to_move, mask) canonicalisation of an object with a ``device`` -- every
class of the package that launches, the boards and the environment included; ``_launches`` puts a whole method inside that context.
``_SearchPolicy``: a policy whose decision is one launch on (state, to_move, mask) -- a subclass supplies ``_run`` (the launch, on
inputs already in the library's form) and gets the batched entry points; ``device`` and ``_lib`` are the subclass's attributes.
``_TreeSearchPolicy``: the targets a tree search leaves in ``last_visits`` / ``last_wins`` / ``last_losses``.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import torch

from . import _native as nat


class _ReferenceAdapters:
    def compute_action(self, obs, mask) -> np.ndarray:  # greedy_policy.py:38-221
        return np.array(int(self.compute_actions(np.asarray(obs)[None], np.asarray(mask)[None])[0]))

    def compute_actions_rllib(self, obs_batch):  # greedy_policy.py:21-31
        observations = np.asarray(obs_batch["observation"])
        observations = observations.reshape(observations.shape[0], 3, 3, -1)
        return list(self.compute_actions(observations, np.asarray(obs_batch["action_mask"])).cpu().numpy())

    def forward(self, batch, state=None, **kwargs):
        """Tianshou-adapter shape (greedy_policy_tianshou.py:63-84): ``batch.obs.obs`` / ``batch.obs.mask``
        (or dict keys "obs" / "mask") for all environments at once -> {"act": int64 (N,)} on the host."""
        ob = batch["obs"] if isinstance(batch, dict) else batch.obs
        obs = ob["obs"] if isinstance(ob, dict) else ob.obs
        mask = ob["mask"] if isinstance(ob, dict) else ob.mask
        act = self.compute_actions(obs, torch.as_tensor(mask).to(torch.int8))
        return {"act": act.to(torch.int64).cpu().numpy()}


def _launches(method):
    """A method of an ``_OnDevice`` class that launches: its whole body runs inside ``_on_device()``."""
    @functools.wraps(method)
    def on_device(self, *args, **kwargs):
        with self._on_device():
            return method(self, *args, **kwargs)
    return on_device


class _OnDevice:
    def _stream(self):
        return nat.current_stream(self.device)

    def _on_device(self):
        """Launches go to the object's device (on its current stream), whichever device is current."""
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    def _inputs(self, state, to_move, mask):
        """(state int8 (N, 27), to_move int8 (N,), mask int8 (N, 54) or None), contiguous on the object's device."""
        state = torch.as_tensor(state).to(device=self.device, dtype=torch.int8).reshape(-1, nat.CELLS).contiguous()
        n = state.shape[0]
        to_move = torch.as_tensor(to_move).to(device=self.device, dtype=torch.int8).reshape(n).contiguous()
        if mask is not None:
            mask = torch.as_tensor(mask).to(device=self.device, dtype=torch.int8).reshape(n, nat.ACTIONS).contiguous()
        return state, to_move, mask


class _SearchPolicy(_OnDevice, _ReferenceAdapters):
    def compute_actions_from_state(self, state, to_move, mask=None) -> torch.Tensor:
        """The decision from ``squares`` (N,27) + ``to_move`` (N,): int32 (N,), -1 where a board has no candidate."""
        return self._run(*self._inputs(state, to_move, mask))

    def compute_actions(self, obs, mask=None) -> torch.Tensor:
        """obs: int8 (N,3,3,13); mask: int8 (N,54) or None (the legal mask of the board)."""
        obs = torch.as_tensor(obs).to(device=self.device, dtype=torch.int8).reshape(-1, 3, 3, 13).contiguous()
        n = obs.shape[0]
        state = torch.empty((n, nat.CELLS), dtype=torch.int8, device=self.device)
        who = torch.empty(n, dtype=torch.int8, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_decode_obs(obs.data_ptr(), state.data_ptr(), who.data_ptr(), n, self._stream()),
                      "gbl_decode_obs")
        return self.compute_actions_from_state(state, who, mask)


class _TreeSearchPolicy(_SearchPolicy):
    """``iterations``: the search's budget; ``_games_per_visit``: how many games' worth of wins / losses one visit of a node adds."""

    def visit_distribution(self, state, to_move, mask=None) -> torch.Tensor:
        """float32 (N, 54): visits / iterations of every root action -- the policy target of a trainer; 0 for non-candidates (one
        call; the decision of the same search is left in ``last_action``)."""
        self.compute_actions_from_state(state, to_move, mask)
        return self.last_visits.to(torch.float32) / self.iterations

    def action_values(self, state, to_move, mask=None) -> torch.Tensor:
        """float32 (N, 54): (W - L) / (n * games per visit) of every visited root action, -inf elsewhere (one call; the decision of
        the same search is left in ``last_action``)."""
        self.compute_actions_from_state(state, to_move, mask)
        seen = self.last_visits > 0
        games = (self.last_visits.clamp(min=1) * self._games_per_visit).to(torch.float32)
        vals = (self.last_wins - self.last_losses).to(torch.float32) / games
        return torch.where(seen, vals, torch.full_like(vals, float("-inf")))
