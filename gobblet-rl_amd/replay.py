"""The device-resident replay buffer: ``ReplayBuffer`` owns a ring of compacted training rows on one device (include/gobblet_hip.h,
"Replay buffer": three arrays of whole 128-byte lines and two counters that live on the device).  ``append`` compacts a collected
window's valid cells into it (``gbl_replay_append``: three launches, nothing waits for the host), ``batch`` draws exactly uniformly
from its newest rows under random symmetries (``gbl_replay_batch``, the dict ``GobbletTrainer.step`` takes) and ``fit`` is the loop of
the two -- on the GPU and, with device="cpu", in the host flavour alike."""
from __future__ import annotations

import torch

from . import _native as nat
from ._policy_base import _OnDevice
from .vector_env import BatchedGobblet

MAX_CAPACITY = (1 << 31) - 1
LINE = 128


def _lines(nbytes: int, device) -> torch.Tensor:
    """`nbytes` zero bytes on `device` that start on a 128-byte line."""
    raw = torch.zeros(nbytes + LINE, dtype=torch.uint8, device=device)
    lead = -raw.data_ptr() % LINE
    return raw[lead:lead + nbytes]


class ReplayBuffer(_OnDevice):
    def __init__(self, capacity: int, device="cuda:0", observations: bool = True) -> None:
        """A ring of ``capacity`` rows (320 bytes each, 192 without observations), empty."""
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError("capacity must be in [1, 2^31 - 1]")
        self.capacity, self.device, self.observations = capacity, torch.device(device), bool(observations)
        self._lib = nat.lib_for(self.device)
        dev = self.device
        self._obs = _lines(capacity * nat.REPLAY_OBS_PITCH, dev).view(torch.int8).view(capacity, nat.REPLAY_OBS_PITCH) if observations else None
        self._visits = _lines(capacity * 2 * nat.REPLAY_VISITS_PITCH, dev).view(torch.int16).view(capacity, nat.REPLAY_VISITS_PITCH)
        self._meta = _lines(capacity * nat.REPLAY_META_PITCH, dev).view(torch.int8).view(capacity, nat.REPLAY_META_PITCH)
        self._state = torch.zeros(2, dtype=torch.int64, device=dev)  # (the ABI's uint64[2]: rows ever appended, rows of the last append)
        self._workspace = None

    # ---- the ring, for inspection: views without the padding (slot order, not age order) ------------------------------------------
    @property
    def observation(self):
        return None if self._obs is None else self._obs[:, :nat.OBS_BYTES]

    @property
    def action_mask(self):
        return self._meta[:, :nat.ACTIONS]

    @property
    def visits(self):
        return self._visits[:, :nat.ACTIONS]

    @property
    def z(self):
        return self._meta[:, nat.REPLAY_META_Z]

    @property
    def mover(self):
        return self._meta[:, nat.REPLAY_META_MOVER]

    @property
    def tag(self):
        return self._meta.view(torch.int32)[:, nat.REPLAY_META_TAG // 4]

    @property
    def total(self) -> int:
        """Rows ever appended.  Reads the device."""
        return int(self._state[0])

    @property
    def size(self) -> int:
        """Rows the buffer holds: min(total, capacity).  Reads the device."""
        return min(self.total, self.capacity)

    def append(self, env: BatchedGobblet, traj: dict, tag: int = 0) -> None:
        """The valid cells of the window ``traj`` of ``env`` (a window with search outputs and ``outcome_targets``: the cells
        ``training_batch`` draws from) go into the ring in ascending (ply, board), overwriting the oldest rows; ``tag`` (an int32, the
        generation for instance) is stored with every row and comes back in a batch's "index".  Waits for nothing."""
        f = traj["_full"]
        if "z" not in f:
            raise ValueError("append needs the 'z' entry: call outcome_targets(traj) first")
        if "visits" not in f or "mover" not in f:
            raise ValueError("append needs a window with search outputs ('visits', 'mover')")
        if f["z"].device != self.device:
            raise ValueError("the window lives on %s and the buffer on %s" % (f["z"].device, self.device))
        if traj["_plies"] < 2:
            raise ValueError("append needs a window of at least 2 plies")
        if self.observations and "observation" not in f:
            raise ValueError("append: the buffer keeps observations and the window has none")
        if not -1 << 31 <= int(tag) < 1 << 31:
            raise ValueError("append: tag must fit an int32")
        n, plies = env.num_envs, traj["_plies"]
        need = nat.lib().gbl_replay_workspace_bytes(n, plies)  # (one function for both flavours: it launches nothing and needs no GPU)
        if self._workspace is None or self._workspace.numel() < need:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_replay_append(
                f["observation"].data_ptr() if self.observations else None, f["action_mask"].data_ptr(), f["visits"].data_ptr(),
                f["z"].data_ptr(), f["done"].data_ptr(), f["mover"].data_ptr(), n, plies, traj["_ply_stride"], traj["_tile_stride"],
                int(tag), nat.ptr(self._obs), self._visits.data_ptr(), self._meta.data_ptr(), self.capacity, self._state.data_ptr(),
                self._workspace.data_ptr(), self._workspace.numel(), self._stream()), "gbl_replay_append")

    def batch(self, batch: int, symmetries="all", call: int = 0, seed: int = 0, recent: int | None = None, out: dict | None = None) -> dict:
        """``batch`` rows drawn exactly uniformly from the newest ``recent`` rows (None: from all the buffer holds), each under a random
        symmetry, one launch of ``gbl_replay_batch``: the keys of ``BatchedGobblet.training_batch`` -- "observation" (a buffer with
        observations), "action_mask", "visits", "z", "sym" -- with "index" int32 (batch, 2) = (slot, tag).  The draws are keyed by
        (``seed``, sample index, ``call``).  An empty buffer gives ``training_batch``'s failed samples (index (-1, -1), zero rows,
        z = ``nat.Z_OPEN``).  ``out``: a dict from an earlier call to write into."""
        if symmetries not in BatchedGobblet.SYMMETRY_MASKS:
            raise ValueError("symmetries: 'all', 'square' or None")
        batch, call, recent = int(batch), int(call), 0 if recent is None else int(recent)
        if batch < 0 or not 0 <= call < 1 << 26:
            raise ValueError("batch: batch >= 0 and 0 <= call < 2^26")
        if recent < 0:
            raise ValueError("batch: recent must be None or >= 0")
        dev = self.device
        spec = {"observation": ((batch, nat.OBS_BYTES), torch.int8), "action_mask": ((batch, nat.ACTIONS), torch.int8),
                "visits": ((batch, nat.ACTIONS), torch.int16), "z": ((batch,), torch.int8), "index": ((batch, 2), torch.int32),
                "sym": ((batch,), torch.int16)}
        if not self.observations:
            del spec["observation"]
        if out is None:
            out = {k: torch.empty(shape, dtype=dtype, device=dev) for k, (shape, dtype) in spec.items()}
        elif set(out) != set(spec) or any(tuple(out[k].shape) != shape or out[k].dtype != dtype or out[k].device != dev
                                          or not out[k].is_contiguous() for k, (shape, dtype) in spec.items()):
            raise ValueError("out: the dict of an earlier batch call of this batch size on this buffer")
        with self._on_device():
            nat.check(self._lib.gbl_replay_batch(
                nat.ptr(self._obs), self._visits.data_ptr(), self._meta.data_ptr(), self.capacity, self._state.data_ptr(), recent, batch,
                BatchedGobblet.SYMMETRY_MASKS[symmetries], int(seed), 0, call, nat.ptr(out.get("observation")),
                out["action_mask"].data_ptr(), out["visits"].data_ptr(), out["z"].data_ptr(), out["index"].data_ptr(),
                out["sym"].data_ptr(), self._stream()), "gbl_replay_batch")
        return out

    def relabel(self, tb, mode: str = "result", count: int = 1, census: bool = False, allow_incomplete: bool = False):
        """Exact targets for the ring's live rows, in place: one launch of ``gbl_tb_targets`` over the ring's own arrays through their
        pitches (``Tablebase.targets`` has the rule).  The live rows are every slot once the ring has wrapped and the first ``total``
        slots before, so a slot never written stays zero; mover bytes, tags and padding are not touched.  Returns the census, int8
        (live rows,) in slot order, when asked.  Reads ``total`` from the device."""
        if self._obs is None:
            raise ValueError("relabel needs a buffer with observations")
        if tb.device != self.device:
            raise ValueError("relabel: the table lives on %s and the buffer on %s" % (tb.device, self.device))
        return tb._targets(self.size, self._obs.data_ptr(), nat.REPLAY_OBS_PITCH, self._meta.data_ptr(), nat.REPLAY_META_PITCH,
                           self._visits.data_ptr(), nat.REPLAY_VISITS_PITCH, self._meta.data_ptr() + nat.REPLAY_META_Z, nat.REPLAY_META_PITCH,
                           mode, count, census, None, allow_incomplete)

    def fit(self, trainer, steps: int, batch: int = 1024, symmetries="all", first_call: int = 0, recent: int | None = None,
            seed: int = 0, targets=None) -> torch.Tensor:
        """``steps`` Adam steps of ``trainer`` (a ``GobbletTrainer`` on this buffer's device): step i draws ``batch(batch, symmetries,
        call=first_call + i, recent=recent)`` into one reused buffer and hands it to ``trainer.step``; nothing crosses to the host.
        ``targets``: a ``Tablebase`` on this device -- every drawn batch goes through ``targets.targets`` first (one more launch per
        step: the fit learns from the exact labels).  Returns the steps' statistics, float32 (steps, 4) on the device, as
        ``BatchedGobblet.fit`` does."""
        if torch.device(trainer.device) != self.device:
            raise ValueError("fit: the trainer lives on %s and the buffer on %s" % (trainer.device, self.device))
        buf, stats = None, []
        for i in range(int(steps)):
            buf = self.batch(batch, symmetries=symmetries, call=int(first_call) + i, seed=seed, recent=recent, out=buf)
            stats.append(trainer.step(buf if targets is None else targets.targets(dict(buf))))
        return torch.stack(stats) if stats else torch.zeros((0, 4), dtype=torch.float32, device=self.device)

    def state_dict(self) -> dict:
        return {"capacity": self.capacity, "observations": self.observations, "state": self._state.clone(), "visits": self._visits.clone(),
                "meta": self._meta.clone(), "obs": None if self._obs is None else self._obs.clone()}

    def load_state_dict(self, state: dict) -> None:
        if int(state["capacity"]) != self.capacity or bool(state["observations"]) != self.observations:
            raise ValueError("load_state_dict: the state is of a buffer with capacity = %d, observations = %s"
                             % (int(state["capacity"]), bool(state["observations"])))
        self._state.copy_(state["state"])
        self._visits.copy_(state["visits"])
        self._meta.copy_(state["meta"])
        if self._obs is not None:
            self._obs.copy_(state["obs"])
