"""``GobbletEvaluator`` -- a small integer network (117 observation bytes -> H hidden units -> 54 action logits and a value) that
the library evaluates INSIDE its kernels, and ``EvaluatorTreeSearchGobbletPolicy`` -- the tree search of ``TreeSearchGobbletPolicy``
with that network in place of the masked-random playouts and with its priors steering the selection (``gbl_evaluate`` /
``gbl_tree_search_eval``, include/gobblet_hip.h).  This is what a network trained on the ``(obs, pi, z)`` targets of
``collect(..., search=...)`` / ``outcome_targets`` is used by: ``GobbletEvaluator.from_float`` quantises a float 117-H-55 MLP.

The rule is integer-only: the kernel and the host flavour (``device="cpu"``) agree bit for bit, and the search draws nothing --
no seed, no call index; two calls on the same boards give the same result -- unless it is asked for root noise (``noise=``,
``gbl_tree_search_eval_noise``): a random row keyed by (seed, board id, call) mixed into the root's prior row, the exploration of
self-play.  ``root_noise`` restates that row in torch for the consumers of a trajectory.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any

import numpy as np
import torch

from . import _native as nat
from ._policy_base import _OnDevice, _TreeSearchPolicy

HIDDEN_SIZES = (64, 128, 192, 256)
OUTPUTS, VALUE = 56, 54
MAX_SHIFT, MAX_B1, MAX_B2 = 24, 1 << 20, 1 << 24
LOG2E_16 = 16.0 * math.log2(math.e)  # a natural-log logit in 1/16 of an octave


def _pow2_at_most(x: float) -> float:
    """The largest power of two s with s <= x (x > 0)."""
    return 2.0 ** math.floor(math.log2(x))


class GobbletEvaluator(_OnDevice):
    """The four integer tensors of a ``gbl_evaluator`` on one device: w1 int8 (117, H), b1 int32 (H,), w2 int8 (H / 4, 56, 4) with
    element [j // 4, k, j % 4] = the weight of hidden unit j for output k, b2 int32 (56,), and the three shifts."""

    def __init__(self, w1, b1, w2, b2, shift1: int, shift_p: int, shift_v: int, device="cpu") -> None:
        self.device = nat.device(device)
        w1, b1, w2, b2 = (torch.as_tensor(t) for t in (w1, b1, w2, b2))
        hidden = int(w1.shape[-1])
        if hidden not in HIDDEN_SIZES:
            raise ValueError("hidden must be 64, 128, 192 or 256")
        if tuple(w1.shape) != (nat.OBS_BYTES, hidden) or tuple(b1.shape) != (hidden,) or tuple(w2.shape) != (hidden // 4, OUTPUTS, 4) \
                or tuple(b2.shape) != (OUTPUTS,):
            raise ValueError("shapes: w1 (117, H), b1 (H,), w2 (H / 4, 56, 4), b2 (56,)")
        for name, sh in (("shift1", shift1), ("shift_p", shift_p), ("shift_v", shift_v)):
            if not 0 <= int(sh) <= MAX_SHIFT:
                raise ValueError(f"{name} must be in [0, {MAX_SHIFT}]")
        if int(b1.abs().max()) > MAX_B1 or int(b2.abs().max()) > MAX_B2:
            raise ValueError("|b1| must not exceed 2^20 and |b2| must not exceed 2^24")
        self.hidden, self.shift1, self.shift_p, self.shift_v = hidden, int(shift1), int(shift_p), int(shift_v)
        # (fresh allocations: 16-byte aligned on either device)
        self.w1 = w1.to(device=self.device, dtype=torch.int8).contiguous().clone()
        self.b1 = b1.to(device=self.device, dtype=torch.int32).contiguous().clone()
        self.w2 = w2.to(device=self.device, dtype=torch.int8).contiguous().clone()
        self.b2 = b2.to(device=self.device, dtype=torch.int32).contiguous().clone()
        self.scales: dict[str, float] = {}  # from_float: the power-of-two scales it chose
        self._lib = nat.lib_for(self.device)

    def to(self, device) -> "GobbletEvaluator":
        ev = GobbletEvaluator(self.w1, self.b1, self.w2, self.b2, self.shift1, self.shift_p, self.shift_v, device=device)
        ev.scales = dict(self.scales)
        return ev

    def as_struct(self) -> nat.Evaluator:
        """The ``gbl_evaluator`` over this object's tensors (keep the object alive while the struct is in use)."""
        return nat.Evaluator(self.w1.data_ptr(), self.b1.data_ptr(), self.w2.data_ptr(), self.b2.data_ptr(), self.hidden, self.shift1,
                             self.shift_p, self.shift_v)

    @staticmethod
    def pack_w2(w2_jk) -> torch.Tensor:
        """(H, 56) -> the (H / 4, 56, 4) layout of the ABI."""
        w2_jk = torch.as_tensor(w2_jk)
        h = w2_jk.shape[0]
        return w2_jk.reshape(h // 4, 4, OUTPUTS).permute(0, 2, 1).contiguous()

    @classmethod
    def from_float(cls, w1, b1, w2, b2, hidden_max: float | None = None, natural_log: bool = True, device="cpu") -> "GobbletEvaluator":
        """Quantise the float network  h = relu(x @ w1 + b1),  out = h @ w2 + b2  with w1 (117, H), b1 (H,), w2 (H, 55), b2 (55,):
        out[:54] are the action logits of a softmax (natural-log if ``natural_log``, else already in 1/16 of an octave), out[54] is
        the value, read as clip(out[54], -1, 1) of a win for the side to move.

        Every scale is a power of two, the largest that keeps the rounded weights inside int8: ``scale1`` for w1 / b1;
        ``scale_h`` = scale1 / 2^shift1 for the hidden units, with shift1 the smallest that keeps ``hidden_max`` (the largest hidden
        activation to represent; default: the bound b1_j + the 21 largest positive weights of unit j) below 128; ``scale_p`` for
        the policy columns after log2(e) * 16 has been folded into them, so that shift_p = log2(scale_p * scale_h) leaves the
        logits in 1/16 of an octave; ``scale_v`` for the value column, shift_v = log2(scale_v * scale_h / 128).  They are kept in
        ``.scales``.  Raises ValueError if a shift leaves 0 .. 24 or a bias its range."""
        w1, b1, w2, b2 = (np.asarray(torch.as_tensor(t).detach().cpu(), np.float64) for t in (w1, b1, w2, b2))
        hidden = w1.shape[1]
        if w1.shape != (nat.OBS_BYTES, hidden) or b1.shape != (hidden,) or w2.shape != (hidden, 55) or b2.shape != (55,):
            raise ValueError("shapes: w1 (117, H), b1 (H,), w2 (H, 55), b2 (55,)")
        scale1 = _pow2_at_most(127.0 / max(float(np.abs(w1).max()), 1e-30))
        if hidden_max is None:
            hidden_max = float((b1 + np.sort(np.maximum(w1, 0.0), axis=0)[-21:].sum(0)).max())
        shift1 = max(0, math.ceil(math.log2(max(hidden_max, 1e-30) * scale1 / 127.0)))
        scale_h = scale1 / 2.0 ** shift1
        fold = LOG2E_16 if natural_log else 1.0
        wp, bp, wv, bv = w2[:, :54] * fold, b2[:54] * fold, w2[:, 54], b2[54]
        scale_p = _pow2_at_most(127.0 / max(float(np.abs(wp).max()), 1e-30))
        scale_v = _pow2_at_most(127.0 / max(float(np.abs(wv).max()), 1e-30))
        shift_p, shift_v = round(math.log2(scale_p * scale_h)), round(math.log2(scale_v * scale_h / 128.0))
        if shift_p > MAX_SHIFT:  # (tiny weights: a smaller scale loses nothing that the shift would not drop)
            scale_p, shift_p = scale_p / 2.0 ** (shift_p - MAX_SHIFT), MAX_SHIFT
        if shift_v > MAX_SHIFT:
            scale_v, shift_v = scale_v / 2.0 ** (shift_v - MAX_SHIFT), MAX_SHIFT
        if shift_p < 0 or shift_v < 0:
            raise ValueError("the output weights are too large for the hidden scale: no shift in [0, 24] represents them")
        q_w1 = np.clip(np.rint(w1 * scale1), -128, 127)
        q_b1 = np.rint(b1 * scale1)
        q_w2 = np.zeros((hidden, OUTPUTS))
        q_w2[:, :54], q_w2[:, VALUE] = np.clip(np.rint(wp * scale_p), -128, 127), np.clip(np.rint(wv * scale_v), -128, 127)
        q_b2 = np.zeros(OUTPUTS)
        q_b2[:54], q_b2[VALUE] = np.rint(bp * scale_p * scale_h), np.rint(bv * scale_v * scale_h)
        ev = cls(torch.from_numpy(q_w1.astype(np.int8)), torch.from_numpy(q_b1.astype(np.int64)),
                 cls.pack_w2(torch.from_numpy(q_w2.astype(np.int8))), torch.from_numpy(q_b2.astype(np.int64)), shift1, shift_p, shift_v,
                 device=device)
        ev.scales = {"scale1": scale1, "scale_h": scale_h, "scale_p": scale_p, "scale_v": scale_v, "fold": fold}
        return ev

    def evaluate_raw(self, state, to_move, mask=None, logits: bool = False):
        """``gbl_evaluate``: (priors uint8 (N, 54), value int32 (N,), logits int32 (N, 56) or None)."""
        state, to_move, mask = self._inputs(state, to_move, mask)
        n = state.shape[0]
        pri = torch.empty((n, nat.ACTIONS), dtype=torch.uint8, device=self.device)
        val = torch.empty(n, dtype=torch.int32, device=self.device)
        log = torch.empty((n, OUTPUTS), dtype=torch.int32, device=self.device) if logits else None
        ev = self.as_struct()
        with self._on_device():
            nat.check(self._lib.gbl_evaluate(state.data_ptr(), to_move.data_ptr(), nat.ptr(mask), C.addressof(ev), pri.data_ptr(),
                                             val.data_ptr(), nat.ptr(log), n, self._stream()), "gbl_evaluate")
        return pri, val, log

    def evaluate(self, state, to_move, mask=None):
        """(priors float32 (N, 54) = pi / sum(pi), zeros where a board has no candidate; value float32 (N,) = q / 128)."""
        pri, val, _ = self.evaluate_raw(state, to_move, mask)
        pri = pri.to(torch.float32)
        return pri / pri.sum(1, keepdim=True).clamp(min=1.0), val.to(torch.float32) / 128.0

    # ---- reanalysis: fresh search targets for stored rows ---------------------------------------------------------------------------
    def _reanalyse(self, n, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z, z_pitch, iterations, explore, census,
                   root_value=None, gumbel=None, seed=0, env_base=0, call=0, gumbel_out=None):
        """One launch of ``gbl_reanalyse`` -- with ``gumbel`` (``gumbel_args``' dict) of ``gbl_reanalyse_gumbel`` -- on ``n`` pitched rows
        (data pointers); returns (drift int32 (n,), census int8 (n,) or None)."""
        for name, val, lo, hi in (("iterations", iterations, 1, 512), ("explore", explore, 0, 1024)):
            if not lo <= int(val) <= hi:
                raise ValueError(f"{name} must be in [{lo}, {hi}]")
        if gumbel is not None:
            if not 0 <= int(call) < 1 << 24:
                raise ValueError("call must be in [0, 2^24)")
            if int(env_base) < 0 or int(env_base) + n > 1 << 42:
                raise ValueError("env_base + the rows must not exceed 2^42")
        drift = torch.empty(n, dtype=torch.int32, device=self.device)
        tally = torch.empty(n, dtype=torch.int8, device=self.device) if census else None
        ev = self.as_struct()
        with self._on_device():
            if gumbel is not None:
                nat.check(self._lib.gbl_reanalyse_gumbel(
                    C.addressof(ev), int(iterations), int(explore), gumbel["considered"], gumbel["noise"], gumbel["visit_offset"],
                    gumbel["scale"], int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_base), int(call), obs, obs_pitch, mask, mask_pitch, visits_in,
                    visits_out, visits_pitch, z, z_pitch, nat.ptr(root_value), None, None, None, drift.data_ptr(), nat.ptr(tally),
                    nat.ptr(gumbel_out), n, self._stream()), "gbl_reanalyse_gumbel")
            else:
                nat.check(self._lib.gbl_reanalyse(C.addressof(ev), int(iterations), int(explore), obs, obs_pitch, mask, mask_pitch, visits_in,
                                                  visits_out, visits_pitch, z, z_pitch, nat.ptr(root_value), None, None, None, drift.data_ptr(),
                                                  nat.ptr(tally), n, self._stream()), "gbl_reanalyse")
        return drift, tally

    def reanalyse(self, batch: dict, iterations: int = 64, explore: int = 16, census: bool = False, out: torch.Tensor | None = None,
                  gumbel: dict | None = None, seed: int = 0, call: int = 0, env_base: int = 0) -> dict:
        """This network's search run again on the rows of the dict ``BatchedGobblet.training_batch`` / ``ReplayBuffer.batch`` return, one
        launch of ``gbl_reanalyse``: returns a copy of the dict whose "visits" are the new search's visit counts (``gbl_tree_search_eval``
        with ``iterations`` and ``explore`` on the position each observation holds, under the row's mask; no noise, no solver guard) in a
        fresh tensor -- or in ``out``, an int16 (N, 54) tensor; ``out=batch["visits"]`` is the in-place form.  "z" stays the game's
        outcome; a failed sample (z = ``nat.Z_OPEN``) keeps its row, a row without a candidate gets zeros.  Adds "root_value" int32 (N,),
        the root's q in 1/128 of a win for the mover, "drift" int32 (N,), the total variation between the old and the new visit shares
        in 1/1024 (1024: the old row had nothing positive; -1: a skipped row or one without a candidate) and, with ``census``, "census"
        int8 (N,) (include/gobblet_hip.h, "Reanalysis": bit 0 the old argmax is the new one, bit 1 the sign of the root's q equals z,
        bit 2 there were no old visits; -1 where drift is).

        gumbel: ``dict(considered=16, noise=True, visit_offset=50, scale=23)`` (``EvaluatorTreeSearchGobbletPolicy``'s keys, defaults and
        checks) makes it one launch of ``gbl_reanalyse_gumbel``: the search is the Gumbel root search, made for budgets such as
        ``iterations=16``, and "visits" become its target rows -- the completed-Q policy, 1 .. 255 on every candidate, what
        ``collect(search=dict(gumbel=...))`` stores.  The noise of row r is keyed by (``seed``, ``env_base`` + r, ``call``);
        ``noise=False`` draws nothing.  Adds "gumbel" int16 (N, 54), the noise g.  "drift" and "census" compare the old row with the
        target row."""
        if "observation" not in batch:
            raise ValueError("reanalyse needs the 'observation' entry: a window or a buffer with observations")
        rule = None if gumbel is None else gumbel_args(gumbel)
        obs, mask, visits, z = batch["observation"], batch.get("action_mask"), batch["visits"], batch["z"]
        n = int(z.shape[0])
        spec = (("observation", obs, (n, nat.OBS_BYTES), torch.int8), ("action_mask", mask, (n, nat.ACTIONS), torch.int8),
                ("visits", visits, (n, nat.ACTIONS), torch.int16), ("z", z, (n,), torch.int8), ("out", out, (n, nat.ACTIONS), torch.int16))
        for name, t, shape, dtype in spec:
            if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"reanalyse: {name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
        if out is None:
            out = visits.clone()  # (a skipped row keeps what it held)
        value = torch.empty(n, dtype=torch.int32, device=self.device)
        noise = None if rule is None else torch.empty((n, nat.ACTIONS), dtype=torch.int16, device=self.device)
        drift, tally = self._reanalyse(n, obs.data_ptr(), nat.OBS_BYTES, nat.ptr(mask), nat.ACTIONS, visits.data_ptr(), out.data_ptr(),
                                       nat.ACTIONS, z.data_ptr(), 1, iterations, explore, census, value, rule, seed, env_base, call, noise)
        fresh = dict(batch, visits=out, root_value=value, drift=drift)
        if census:
            fresh["census"] = tally
        if rule is not None:
            fresh["gumbel"] = noise
        return fresh


class EvaluatorTreeSearchGobbletPolicy(_TreeSearchPolicy):
    _games_per_visit = 128  # (a network leaf counts as 128 games)

    def __init__(self, evaluator: GobbletEvaluator, iterations: int = 256, explore: int = 16, noise: float = 0.0, seed: int = 0,
                 env_base: int = 0, device=None, gumbel: dict | None = None, **kwargs: Any) -> None:
        """iterations: network leaves per decision (1 .. 512); explore: weight of the prior term of the selection key (0 .. 1024;
        the default is the best of the host-flavour sweep in profiles/r10/evaluator_policy.json); device: where the search runs
        (default: the evaluator's; the evaluator is copied there if it lives elsewhere).

        noise: the share in [0, 1] of a random row mixed into the ROOT's prior row, once per search (``gbl_tree_search_eval_noise``;
        the weight of the ABI is round(256 * noise)).  The row of board b of call k is keyed by (seed, env_base + b, k): ``call``
        counts up once per ``compute_actions_from_state``.  With noise 0 the policy draws nothing.

        gumbel: ``dict(considered=16, noise=True, visit_offset=50, scale=23)`` (any key may be left out) makes the ROOT follow the
        Gumbel rule (``gbl_tree_search_gumbel``), the search for small budgets such as ``iterations=16``: Gumbel noise once per root
        (keyed like the root noise; ``noise=False``: none, the policy draws nothing), the ``considered`` (1 .. 54) best actions by
        noise + logit, sequential halving over them, the decision among the survivors.  ``visit_offset`` (0 .. 255) and ``scale``
        (0 .. 64, in 1/16 of an octave per unit of value) are the paper's c_visit and c_scale; the defaults are its 50 and 1.0 nat.
        ``last_target`` is then the completed-Q improved policy, uint8 (N, 54), and ``last_gumbel`` the noise, int16 (N, 54).  Not
        together with ``noise``."""
        for name, val, lo, hi in (("iterations", iterations, 1, 512), ("explore", explore, 0, 1024)):
            if not lo <= int(val) <= hi:
                raise ValueError(f"{name} must be in [{lo}, {hi}]")
        self.iterations, self.explore = int(iterations), int(explore)
        self.noise = noise_weight(noise)
        self.gumbel = None if gumbel is None else gumbel_args(gumbel)
        if self.gumbel is not None and self.noise:
            raise ValueError("gumbel does not go with noise: the Gumbel row is the search's exploration")
        self.seed, self.env_base, self.call = int(seed), int(env_base), 0
        self.device = nat.device(evaluator.device if device is None else device)
        self.evaluator = evaluator if evaluator.device == self.device else evaluator.to(self.device)
        self._lib = nat.lib_for(self.device)
        # outputs of the last call (tensors on the device): int32 (N, 54) visits / wins / losses of the root's children from the
        # mover's side (a leaf counts as 128 games), int32 (N,) nodes created, the decision and the root's q, uint8 (N, 54) the
        # root's prior row as the network gives it, and as the root keeps it (the same row without noise)
        self.last_visits = self.last_wins = self.last_losses = self.last_nodes = self.last_action = None
        self.last_root_value = self.last_root_priors = self.last_root_mixed = None
        self.last_target = self.last_gumbel = None  # (gumbel=: the target row uint8 (N, 54) and the noise int16 (N, 54))

    def _run(self, state, to_move, mask) -> torch.Tensor:
        n = state.shape[0]
        visits = torch.empty((n, nat.ACTIONS), dtype=torch.int32, device=self.device)
        wins, losses = torch.empty_like(visits), torch.empty_like(visits)
        act = torch.empty(n, dtype=torch.int32, device=self.device)
        nodes, rootv = torch.empty_like(act), torch.empty_like(act)
        rootp = torch.empty((n, nat.ACTIONS), dtype=torch.uint8, device=self.device)
        mixed = rootp
        ev = self.evaluator.as_struct()
        target = gum = None
        with self._on_device():
            if self.gumbel is not None:
                target, gum = torch.empty_like(rootp), torch.empty((n, nat.ACTIONS), dtype=torch.int16, device=self.device)
                g = self.gumbel
                nat.check(self._lib.gbl_tree_search_gumbel(
                    state.data_ptr(), to_move.data_ptr(), nat.ptr(mask), C.addressof(ev), self.iterations, self.explore, g["considered"],
                    g["noise"], g["visit_offset"], g["scale"], self.seed, self.env_base, self.call, visits.data_ptr(), wins.data_ptr(),
                    losses.data_ptr(), act.data_ptr(), nodes.data_ptr(), rootv.data_ptr(), rootp.data_ptr(), target.data_ptr(),
                    gum.data_ptr(), n, self._stream()), "gbl_tree_search_gumbel")
                self.call += 1
            elif self.noise:
                mixed = torch.empty_like(rootp)
                nat.check(self._lib.gbl_tree_search_eval_noise(
                    state.data_ptr(), to_move.data_ptr(), nat.ptr(mask), C.addressof(ev), self.iterations, self.explore, self.noise,
                    self.seed, self.env_base, self.call, visits.data_ptr(), wins.data_ptr(), losses.data_ptr(), act.data_ptr(),
                    nodes.data_ptr(), rootv.data_ptr(), rootp.data_ptr(), mixed.data_ptr(), n, self._stream()),
                    "gbl_tree_search_eval_noise")
                self.call += 1
            else:
                nat.check(self._lib.gbl_tree_search_eval(state.data_ptr(), to_move.data_ptr(), nat.ptr(mask), C.addressof(ev),
                                                         self.iterations, self.explore, visits.data_ptr(), wins.data_ptr(),
                                                         losses.data_ptr(), act.data_ptr(), nodes.data_ptr(), rootv.data_ptr(),
                                                         rootp.data_ptr(), n, self._stream()), "gbl_tree_search_eval")
        self.last_visits, self.last_wins, self.last_losses = visits, wins, losses
        self.last_nodes, self.last_action, self.last_root_value, self.last_root_priors = nodes, act, rootv, rootp
        self.last_root_mixed = mixed
        self.last_target, self.last_gumbel = target, gum
        return act


def noise_weight(noise) -> int:
    """The ABI's weight 0 .. 256 of a noise share in [0, 1]."""
    if not 0.0 <= float(noise) <= 1.0:
        raise ValueError("noise must be in [0, 1]")
    return int(round(256.0 * float(noise)))


# ---- the root noise restated in torch (include/gobblet_hip.h, "Root noise"): a convenience for consumers, not a kernel -----------
_EXP2_16 = (65536, 62757, 60097, 57549, 55109, 52773, 50535, 48393, 46341, 44376, 42495, 40693, 38968, 37316, 35734, 34219)
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def _philox4x32_10(c, k0: int, k1: int):
    """Philox4x32-10 on int64 tensors that hold 32-bit words: c = [c0, c1, c2, c3] -> the four output words."""
    def mulhilo(m: int, x):
        lo, hi = x & 0xFFFF, x >> 16          # (x * m in two halves: every product stays below 2^63)
        ml, mh = m & 0xFFFF, m >> 16
        ll, lh, hl, hh = lo * ml, lo * mh, hi * ml, hi * mh
        mid = (ll >> 16) + (lh & 0xFFFF) + (hl & 0xFFFF)
        return (hh + (lh >> 16) + (hl >> 16) + (mid >> 16)) & _M32, ((mid << 16) | (ll & 0xFFFF)) & _M32
    c0, c1, c2, c3 = c
    for _ in range(10):
        hi0, lo0 = mulhilo(_PHILOX_M0, c0)
        hi1, lo1 = mulhilo(_PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def root_noise(seed: int, board_ids, ply, candidates) -> torch.Tensor:
    """uint8 (N, 54): the noise rows nu of ``gbl_tree_search_eval_noise`` / ``gbl_collect_search_noise`` for boards ``board_ids``
    (N,) (= env_base + b) at call / ply index ``ply`` (an int or (N,)) over the candidate sets ``candidates`` (N, 54), non-zero =
    candidate -- the legal mask of an unguarded side, the outcome-0 actions of a guarded one.  A consumer of a trajectory rebuilds
    the row the root kept from "priors":  pi' = (pi * (256 - w) + nu * w + 128) >> 8.  On the device of ``candidates``."""
    cand = torch.as_tensor(candidates)
    dev = cand.device
    cand = cand.reshape(-1, nat.ACTIONS) != 0
    n = cand.shape[0]
    g = torch.as_tensor(board_ids, device=dev).to(torch.int64).reshape(-1).expand(n)
    q = torch.as_tensor(ply, device=dev).to(torch.int64).reshape(-1).expand(n)
    a = torch.arange(nat.ACTIONS, device=dev, dtype=torch.int64)
    idx = (64 * q)[:, None] + a[None, :]                      # the ply index 64 q + a
    blk = idx[:, 0::4] >> 2                                   # one block per four actions: (N, 14)
    zero = torch.zeros_like(blk)
    words = _philox4x32_10([(g & _M32)[:, None] + zero, (g >> 32)[:, None] + zero, blk, zero + nat.STREAM_NOISE],
                           int(seed) & _M32, (int(seed) >> 32) & _M32)
    r = torch.stack(words, dim=2).reshape(n, 56)[:, :nat.ACTIONS] >> 24
    rmin = torch.where(cand, r, torch.full_like(r, 255)).min(1, keepdim=True).values
    d = (r - rmin).clamp(min=0)
    e = torch.tensor(_EXP2_16, device=dev, dtype=torch.int64)[d & 15] >> (d >> 4)
    e = torch.where(cand, e, torch.zeros_like(e))
    nu = 1 + (e * 254) // e.sum(1, keepdim=True).clamp(min=1)
    return torch.where(cand, nu, torch.zeros_like(nu)).to(torch.uint8)


# ---- the playout cap's draw restated in torch (include/gobblet_hip.h, gbl_collect_search_cap): a convenience, not a kernel ----------
def cap_share(full) -> int:
    """The ABI's share 0 .. 256 of full plies for a share in [0, 1]."""
    if not 0.0 <= float(full) <= 1.0:
        raise ValueError("cap: full must be in [0, 1]")
    return int(round(256.0 * float(full)))


def cap_full(seed: int, board_ids, ply_indices, full) -> torch.Tensor:
    """bool: which plies of ``gbl_collect_search_cap`` are FULL for a side whose share of full plies is ``full`` (in [0, 1], as
    ``collect(search=dict(cap=dict(full=...)))`` takes it).  ``board_ids`` (= env_base + b) and ``ply_indices`` broadcast against
    each other: ``cap_full(seed, ids[None, :], plies[:, None], 0.25)`` has a time-major trajectory's shape.  The draw alone: a ply
    of a side that does not search, and a ply the solver proves, takes none.  On the device of ``board_ids``."""
    share = cap_share(full)
    g = torch.as_tensor(board_ids)
    dev = g.device
    g, q = torch.broadcast_tensors(g.to(torch.int64), torch.as_tensor(ply_indices, device=dev).to(torch.int64))
    zero = torch.zeros_like(g)
    words = _philox4x32_10([g & _M32, g >> 32, q >> 2, zero + nat.STREAM_CAP], int(seed) & _M32, (int(seed) >> 32) & _M32)
    r = torch.stack(words, dim=-1).gather(-1, (q & 3)[..., None])[..., 0]
    return (r >> 24) < share


# ---- the Gumbel root rule's arguments and its noise restated in torch (include/gobblet_hip.h, "Gumbel root search") ------------------
GUMBEL_DEFAULTS = dict(considered=16, noise=True, visit_offset=50, scale=23)
GUMBEL_TABLE_KEYS = ("tablebase", "tb_mode", "tb_count", "judge", "allow_incomplete")  # collect()'s gumbel dict alone: the table inside it
# GT[k] = round(-ln(-ln((k + 1/2) / 256)) * 16 / ln 2): a standard Gumbel variate in 1/16 of an octave (csrc/gobblet_knobs.h holds the numbers)
GUMBEL_TABLE = tuple(int(x) for x in np.rint(-np.log(-np.log((np.arange(256) + 0.5) / 256.0)) * 16.0 / math.log(2.0)))


def gumbel_args(gumbel: dict) -> dict:
    """``gumbel=dict(...)`` with the defaults filled in, as the ABI takes it: considered 1 .. 54, noise 0 / 1, visit_offset 0 .. 255,
    scale 0 .. 64."""
    if isinstance(gumbel, dict) and "solve_depth" in gumbel:  # (collect()'s gumbel dict alone has the key: gbl_collect_gumbel_solve)
        raise ValueError("gumbel: solve_depth belongs to collect(search=dict(gumbel=...)); a single decision is guarded by "
                         "SolverGobbletPolicy(depth, fallback=this policy)")
    if isinstance(gumbel, dict) and set(gumbel) & set(GUMBEL_TABLE_KEYS):  # (likewise: gbl_collect_gumbel_tb)
        raise ValueError("gumbel: tablebase / tb_mode / tb_count / judge / allow_incomplete belong to collect(search=dict(gumbel=...)); "
                         "a single decision plays from the table through TablebaseGobbletPolicy(tb, fallback=this policy)")
    if not isinstance(gumbel, dict) or set(gumbel) - set(GUMBEL_DEFAULTS):
        raise ValueError("gumbel is a dict of considered / noise / visit_offset / scale")
    kw = {**GUMBEL_DEFAULTS, **gumbel}
    out = {"noise": int(bool(kw["noise"]))}
    if kw["noise"] not in (0, 1, False, True):
        raise ValueError("gumbel: noise is True or False")
    for name, lo, hi in (("considered", 1, 54), ("visit_offset", 0, 255), ("scale", 0, 64)):
        v = kw[name]
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
            raise ValueError(f"gumbel: {name} must be an integer in [{lo}, {hi}]")
        out[name] = int(v)
    return out


def gumbel_row(seed: int, board_ids, ply) -> torch.Tensor:
    """int16 (N, 54): the Gumbel values g of ``gbl_tree_search_gumbel`` / ``gbl_collect_search_gumbel`` (with noise) for boards
    ``board_ids`` (N,) (= env_base + b) at call / ply index ``ply`` (an int or (N,)), for EVERY action: the entry points write them for
    the root's candidates and 0 elsewhere.  On the device of ``board_ids``."""
    g = torch.as_tensor(board_ids)
    dev = g.device
    g = g.to(torch.int64).reshape(-1)
    n = g.shape[0]
    q = torch.as_tensor(ply, device=dev).to(torch.int64).reshape(-1).expand(n)
    a = torch.arange(nat.ACTIONS, device=dev, dtype=torch.int64)
    blk = ((64 * q)[:, None] + a[None, 0::4]) >> 2            # one block per four actions: (N, 14)
    zero = torch.zeros_like(blk)
    words = _philox4x32_10([(g & _M32)[:, None] + zero, (g >> 32)[:, None] + zero, blk, zero + nat.STREAM_GUMBEL],
                           int(seed) & _M32, (int(seed) >> 32) & _M32)
    r = torch.stack(words, dim=2).reshape(n, 56)[:, :nat.ACTIONS] >> 24
    return torch.tensor(GUMBEL_TABLE, device=dev, dtype=torch.int16)[r]
