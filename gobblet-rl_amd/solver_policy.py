"""``SolverGobbletPolicy`` -- the exact bounded-depth solver for N boards at once: the full-width game tree of every board to
``depth`` plies, one launch of ``gbl_solve`` per call (include/gobblet_hip.h).  Where every other policy of the package estimates,
this one proves: ``outcomes`` gives, for every legal action, +k (the mover wins at ply k against every defence), -k (the mover has
lost by ply k whatever they do) or 0 (nothing is proven within ``depth`` plies), and the decision is the shortest forced win, else
an unproven action, else the longest forced loss.  Integer-only and deterministic: the kernel and the host flavour
(``device="cpu"``) agree byte for byte.

The surface mirrors the other policies (``compute_actions`` / ``compute_actions_from_state`` / ``compute_action`` /
``compute_actions_rllib`` / ``forward``).  A solver knows nothing about an unproven position, so by itself it plays the LOWEST
unproven action there; ``fallback=`` hands those boards to another policy, restricted to the unproven actions:

    G.SolverGobbletPolicy(4, fallback=G.EvaluatorTreeSearchGobbletPolicy(ev, 64))   # never misses a win in 3, never walks into a loss in 4
"""
from __future__ import annotations

from typing import Any

import torch

from . import _native as nat
from ._policy_base import _SearchPolicy


class SolverGobbletPolicy(_SearchPolicy):
    def __init__(self, depth: int = 4, device="cuda:0", fallback=None, **kwargs: Any) -> None:
        """depth: plies searched (1 .. 6; the cost grows by about the branching factor, ~25, per ply).  fallback: a policy instance
        of this package on the same device (anything with ``compute_actions_from_state(state, to_move, mask)``) that decides the
        boards whose root is unproven, among their unproven actions."""
        if not 1 <= int(depth) <= nat.SOLVE_MAX_DEPTH:
            raise ValueError(f"depth must be in [1, {nat.SOLVE_MAX_DEPTH}]")
        self.depth = int(depth)
        self.device = nat.device(device)
        if fallback is not None and nat.device(fallback.device) != self.device:
            raise ValueError("the fallback policy must live on the solver's device")
        self.fallback = fallback
        self._lib = nat.lib_for(self.device)  # ("cpu": the host flavour of the ABI, asked for -- never a fallback)
        # outputs of the last call (tensors on the device): int8 (N, 54) the result of every candidate (nat.SOLVE_NONE elsewhere),
        # int8 (N,) the root's value, int32 (N,) the solver's own decision (before any fallback)
        self.last_outcomes = self.last_value = self.last_action = None

    def _run(self, state: torch.Tensor, to_move: torch.Tensor, mask) -> torch.Tensor:
        n = state.shape[0]
        outcome = torch.empty((n, nat.ACTIONS), dtype=torch.int8, device=self.device)
        value = torch.empty(n, dtype=torch.int8, device=self.device)
        act = torch.empty(n, dtype=torch.int32, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_solve(state.data_ptr(), to_move.data_ptr(), nat.ptr(mask), self.depth, outcome.data_ptr(),
                                          value.data_ptr(), act.data_ptr(), n, self._stream()), "gbl_solve")
        self.last_outcomes, self.last_value, self.last_action = outcome, value, act
        return act

    def compute_actions_from_state(self, state, to_move, mask=None) -> torch.Tensor:
        """The decision from ``squares`` (N,27) + ``to_move`` (N,): int32 (N,), -1 where a board has no candidate.  A proven root
        (``last_value`` != 0) gets the solver's action: the shortest win, or the longest loss.  An UNPROVEN root (value 0) gets the
        contract's ``action_out`` -- the lowest-index action whose outcome is 0, which is no judgement of that action -- unless a
        ``fallback`` policy was given: then the fallback decides those boards, its ``mask`` argument restricted to the actions
        whose outcome is 0, so it can neither pass over a proven win nor pick a proven loss."""
        state, to_move, mask = self._inputs(state, to_move, mask)
        act = self._run(state, to_move, mask)
        if self.fallback is None:
            return act
        open_ = (self.last_outcomes == 0).to(torch.int8)
        unproven = open_.any(1) & (self.last_value == 0)
        if bool(unproven.any()):
            rows = torch.nonzero(unproven).reshape(-1)
            theirs = self.fallback.compute_actions_from_state(state[rows], to_move[rows], open_[rows])
            act = act.clone()
            act[rows] = theirs.to(device=self.device, dtype=torch.int32)
        return act

    def outcomes(self, state, to_move, mask=None) -> torch.Tensor:
        """int8 (N, 54): the proven result of every candidate action, ``nat.SOLVE_NONE`` (-128) elsewhere (one call; the value and the
        solver's decision of the same search are left in ``last_value`` / ``last_action``)."""
        self._run(*self._inputs(state, to_move, mask))
        return self.last_outcomes
