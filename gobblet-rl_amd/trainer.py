"""The float trainer of the evaluator: ``GobbletTrainer`` owns the 117-H-55 network ``GobbletEvaluator.from_float`` quantises, its Adam
moments and the workspace on one device, and ``step`` is one call of ``gbl_train_step`` (include/gobblet_hip.h: two launches, every
float operation in a stated order, so that a fit is reproducible bit for bit from a seed -- on the GPU and, with device="cpu", in the
host flavour alike)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from ._policy_base import _OnDevice
from .evaluator_policy import HIDDEN_SIZES, GobbletEvaluator

OUTPUTS = 55  # 54 action logits and the value
MAX_BATCH = 65536


def param_count(hidden: int) -> int:
    return (nat.OBS_BYTES + 1 + OUTPUTS) * hidden + OUTPUTS


class GobbletTrainer(_OnDevice):
    def __init__(self, hidden: int = 64, device="cuda:0", lr: float = 2e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-4, value_reg: float = 1e-2, seed: int = 0) -> None:
        """The network starts as ``torch.nn.Linear(117, hidden)`` and ``torch.nn.Linear(hidden, 55)`` do after
        ``torch.manual_seed(seed)``, drawn on the host (the caller's generator is left alone); the loss and the optimiser are those of
        ``examples/example_train_evaluator.py``: cross-entropy of the visit shares + (clip(value) - z)^2 + value_reg * value^2, Adam
        with L2 weight decay."""
        if hidden not in HIDDEN_SIZES:
            raise ValueError("hidden must be 64, 128, 192 or 256")
        self.hidden, self.device = int(hidden), nat.device(device)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.weight_decay, self.value_reg = float(weight_decay), float(value_reg)
        self._lib = nat.lib_for(self.device)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(int(seed))
            l1, l2 = torch.nn.Linear(nat.OBS_BYTES, hidden), torch.nn.Linear(hidden, OUTPUTS)
        with torch.no_grad():
            flat = torch.cat([l1.weight.T.reshape(-1), l1.bias, l2.weight.T.reshape(-1), l2.bias]).to(torch.float32)
        # (fresh allocations: 16-byte aligned on either device)
        self.params = flat.to(self.device).contiguous().clone()
        self.m, self.v = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.last_grad = torch.zeros_like(self.params)  # the gradient the last step's Adam consumed (for tests)
        self.hidden_max = torch.zeros((), dtype=torch.float32, device=self.device)  # the largest hidden activation any step has seen
        self.t = 0
        self._workspace = None
        self.last_row_loss = None  # float32 (B, 2): the rows' unweighted (policy, value) losses of the last weighted step
        self.last_priority = None  # int32 (B,): the priorities the last step(priority=...) made of them

    def step(self, batch: dict, weights: torch.Tensor | None = None, priority: dict | None = None) -> torch.Tensor:
        """One Adam step on the dict ``BatchedGobblet.training_batch`` returns ("observation", "action_mask", "visits", "z"; without
        "action_mask" every action is a candidate).  Returns float32 (4,) on the device: the mean policy loss, the mean value loss
        (with its value_reg term), the number of rows that counted and the largest hidden activation over them; nothing waits for the
        device.
        ``weights`` (float32 (B,) on the trainer's device) and ``priority`` (``dict(scale=, floor=1, cap=)``): with either the step is
        ``gbl_train_step_weighted``'s -- row r's loss and gradient count ``weights[r]`` times (the means stay over the counted rows),
        ``last_row_loss`` holds the rows' unweighted losses and, with ``priority``, ``last_priority`` holds
        min(floor + int((policy loss + value loss) * scale), cap) per counted row and 0 for the others: what
        ``ReplayBuffer.set_priority`` takes.  Both are buffers the next such step overwrites."""
        if "observation" not in batch:
            raise ValueError("step needs the 'observation' entry: a window collected with observations")
        obs, mask, visits, z = batch["observation"], batch.get("action_mask"), batch["visits"], batch["z"]
        n = int(z.shape[0])
        if not 1 <= n <= MAX_BATCH:
            raise ValueError(f"step: the batch must hold 1 .. {MAX_BATCH} rows")
        spec = (("observation", obs, (n, nat.OBS_BYTES), torch.int8), ("action_mask", mask, (n, nat.ACTIONS), torch.int8),
                ("visits", visits, (n, nat.ACTIONS), torch.int16), ("z", z, (n,), torch.int8))
        for name, t, shape, dtype in spec:
            if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"step: {name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
        extra = None if weights is None and priority is None else self._weighted_arguments(n, weights, priority)
        need = nat.lib().gbl_train_workspace_bytes(n, self.hidden)  # (one function for both flavours: it launches nothing and needs no GPU)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.t += 1
        b1, b2 = self.betas
        hyper = nat.TrainHyper(self.lr, b1, b2, self.eps, self.weight_decay, self.value_reg, 1.0 - b1 ** self.t, 1.0 - b2 ** self.t)
        stats = torch.empty(4, dtype=torch.float32, device=self.device)
        if extra is not None:
            with self._on_device():
                nat.check(self._lib.gbl_train_step_weighted(
                    obs.data_ptr(), nat.ptr(mask), visits.data_ptr(), z.data_ptr(), n, self.hidden, self.params.data_ptr(), self.m.data_ptr(),
                    self.v.data_ptr(), C.addressof(hyper), nat.ptr(weights), self.last_row_loss.data_ptr(),
                    None if priority is None else self.last_priority.data_ptr(), *extra, self.last_grad.data_ptr(), stats.data_ptr(),
                    self._workspace.data_ptr(), self._workspace.numel(), self._stream()), "gbl_train_step_weighted")
                torch.maximum(self.hidden_max, stats[3], out=self.hidden_max)
            return stats
        with self._on_device():
            nat.check(self._lib.gbl_train_step(obs.data_ptr(), nat.ptr(mask), visits.data_ptr(), z.data_ptr(), n, self.hidden,
                                               self.params.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), C.addressof(hyper),
                                               self.last_grad.data_ptr(), stats.data_ptr(), self._workspace.data_ptr(),
                                               self._workspace.numel(), self._stream()), "gbl_train_step")
            torch.maximum(self.hidden_max, stats[3], out=self.hidden_max)
        return stats

    def _weighted_arguments(self, n, weights, priority):
        """Checks ``step``'s two optional arguments, sizes the two reused output buffers and returns (scale, floor, cap)."""
        if weights is not None and (tuple(weights.shape) != (n,) or weights.dtype != torch.float32 or weights.device != self.device
                                    or not weights.is_contiguous()):
            raise ValueError(f"step: weights must be a contiguous float32 tensor of shape ({n},) on {self.device}")
        scale, floor, cap = 0.0, 0, 0
        if priority is not None:
            if set(priority) - {"scale", "floor", "cap"} or "scale" not in priority or "cap" not in priority:
                raise ValueError("step: priority is dict(scale=, floor=1, cap=)")
            scale, floor, cap = float(priority["scale"]), int(priority.get("floor", 1)), int(priority["cap"])
            if not (0.0 <= scale < float("inf")) or not 0 <= floor <= cap < 1 << 31:
                raise ValueError("step: priority needs a finite scale >= 0 and 0 <= floor <= cap < 2^31")
            if self.last_priority is None or self.last_priority.shape[0] != n:
                self.last_priority = torch.empty(n, dtype=torch.int32, device=self.device)
        if self.last_row_loss is None or self.last_row_loss.shape[0] != n:
            self.last_row_loss = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        return scale, floor, cap

    def weights(self):
        """(w1 (117, H), b1 (H,), w2 (H, 55), b2 (55,)): views of the parameter vector in ``from_float``'s shapes."""
        h, p = self.hidden, self.params
        a, b, c = nat.OBS_BYTES * h, (nat.OBS_BYTES + 1) * h, (nat.OBS_BYTES + 1 + OUTPUTS) * h
        return p[:a].view(nat.OBS_BYTES, h), p[a:b], p[b:c].view(h, OUTPUTS), p[c:]

    def evaluator(self, device=None) -> GobbletEvaluator:
        """The integer evaluator of the current weights, scaled for the largest hidden activation the steps have seen (before the
        first step: ``from_float``'s own bound).  Reads the device."""
        top = float(self.hidden_max)
        return GobbletEvaluator.from_float(*self.weights(), hidden_max=top if top > 0.0 else None,
                                           device=self.device if device is None else device)

    def state_dict(self) -> dict:
        return {"hidden": self.hidden, "t": self.t, "params": self.params.clone(), "m": self.m.clone(), "v": self.v.clone(),
                "hidden_max": self.hidden_max.clone()}

    def load_state_dict(self, state: dict) -> None:
        if int(state["hidden"]) != self.hidden:
            raise ValueError("load_state_dict: the state is of a network with hidden = %d" % int(state["hidden"]))
        for name in ("params", "m", "v", "hidden_max"):
            getattr(self, name).copy_(state[name])
        self.t = int(state["t"])
