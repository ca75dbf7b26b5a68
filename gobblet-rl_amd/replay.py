"""The device-resident replay buffer: ``ReplayBuffer`` owns a ring of compacted training rows on one device (include/gobblet_hip.h,
"Replay buffer": three arrays of whole 128-byte lines and two counters that live on the device).  ``append`` compacts a collected
window's valid cells into it (``gbl_replay_append``: three launches, nothing waits for the host), ``batch`` draws exactly uniformly
from its newest rows under random symmetries (``gbl_replay_batch``, the dict ``GobbletTrainer.step`` takes) and ``fit`` is the loop of
the two -- on the GPU and, with device="cpu", in the host flavour alike.  With ``prioritized=True`` the buffer also owns a priority per
row and the index of their prefix sums: ``append`` sets the new rows' priorities, ``set_priority`` / ``set_all_priority`` change them,
``batch(prioritized=True)`` draws with probability proportional to them (``gbl_replay_batch_prio``, one launch, after a rebuild of the index
on the same stream when anything changed since the last one)."""
from __future__ import annotations

import torch

from . import _native as nat
from ._policy_base import _OnDevice
from .evaluator_policy import gumbel_args
from .vector_env import BatchedGobblet

MAX_CAPACITY = (1 << 31) - 1
LINE = 128


def _lines(nbytes: int, device) -> torch.Tensor:
    """`nbytes` zero bytes on `device` that start on a 128-byte line."""
    raw = torch.zeros(nbytes + LINE, dtype=torch.uint8, device=device)
    lead = -raw.data_ptr() % LINE
    return raw[lead:lead + nbytes]


class ReplayBuffer(_OnDevice):
    def __init__(self, capacity: int, device="cuda:0", observations: bool = True, prioritized: bool = False) -> None:
        """A ring of ``capacity`` rows (320 bytes each, 192 without observations), empty.  ``prioritized``: 4 more bytes per row for its
        priority (all zeros: a row is drawn by priority only once it has been given one) and the index, 8 bytes per 32 rows."""
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError("capacity must be in [1, 2^31 - 1]")
        self.capacity, self.device, self.observations = capacity, nat.device(device), bool(observations)
        self._lib = nat.lib_for(self.device)
        dev = self.device
        self._obs = _lines(capacity * nat.REPLAY_OBS_PITCH, dev).view(torch.int8).view(capacity, nat.REPLAY_OBS_PITCH) if observations else None
        self._visits = _lines(capacity * 2 * nat.REPLAY_VISITS_PITCH, dev).view(torch.int16).view(capacity, nat.REPLAY_VISITS_PITCH)
        self._meta = _lines(capacity * nat.REPLAY_META_PITCH, dev).view(torch.int8).view(capacity, nat.REPLAY_META_PITCH)
        self._state = torch.zeros(2, dtype=torch.int64, device=dev)  # (the ABI's uint64[2]: rows ever appended, rows of the last append)
        self._workspace = None
        self.prioritized = bool(prioritized)
        if self.prioritized:
            self._prio = _lines(4 * capacity, dev).view(torch.int32)
            self._index = _lines(nat.lib().gbl_replay_prio_index_bytes(capacity), dev).view(torch.int64)
            self._index_current = False  # (host bookkeeping alone: append and every priority write clear it, a prioritised draw rebuilds)
            self._cells = None

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
    def priority(self):
        """int32 (capacity,), slot order; a row's weight is max(priority, 0).  A view: write through ``set_priority`` /
        ``set_all_priority``, which know that the index is stale afterwards."""
        self._need_priorities("priority")
        return self._prio

    def _need_priorities(self, what: str) -> None:
        if not self.prioritized:
            raise ValueError("%s needs ReplayBuffer(..., prioritized=True)" % what)

    @property
    def total(self) -> int:
        """Rows ever appended.  Reads the device."""
        return int(self._state[0])

    @property
    def size(self) -> int:
        """Rows the buffer holds: min(total, capacity).  Reads the device."""
        return min(self.total, self.capacity)

    def append(self, env: BatchedGobblet, traj: dict, tag: int = 0, priority=1) -> None:
        """The valid cells of the window ``traj`` of ``env`` (a window with search outputs and ``outcome_targets``: the cells
        ``training_batch`` draws from) go into the ring in ascending (ply, board), overwriting the oldest rows; ``tag`` (an int32, the
        generation for instance) is stored with every row and comes back in a batch's "index".  Waits for nothing.
        ``priority`` (a prioritised buffer only): the new rows' priority, an int or an integer tensor per cell shaped like ``traj["z"]``
        (one more launch, ``gbl_replay_prio_append``).  A row takes the value of the cell its visits come from: ply t's cell, which is
        also the cell of ``Tablebase.judge``'s "regret" and "z_exact" (the judge arrays describe ply t's position and mover, as "visits"
        does), so ``priority=table[traj["regret"].long() + 1]`` with a small weight table is the intended use."""
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
        prio_traj = None
        if self.prioritized:
            if isinstance(priority, torch.Tensor):
                if priority.shape != traj["z"].shape or priority.is_floating_point() or priority.device != self.device:
                    raise ValueError("append: priority must be an int or an integer tensor shaped like traj['z'] on the buffer's device")
                if self._cells is None or self._cells.shape != f["z"].shape:
                    self._cells = torch.zeros(f["z"].shape, dtype=torch.int32, device=self.device)
                (self._cells[:, :env.num_envs] if traj["_layout"] == "time" else self._cells).copy_(priority)
                prio_traj, priority = self._cells, 0
            elif not -1 << 31 <= int(priority) < 1 << 31:
                raise ValueError("append: priority must fit an int32")
        elif isinstance(priority, torch.Tensor) or int(priority) != 1:
            self._need_priorities("append(priority=...)")
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
            if self.prioritized:
                self._index_current = False
                nat.check(self._lib.gbl_replay_prio_append(
                    f["visits"].data_ptr(), f["z"].data_ptr(), f["done"].data_ptr(), nat.ptr(prio_traj), int(priority), n, plies,
                    traj["_ply_stride"], traj["_tile_stride"], self._prio.data_ptr(), self.capacity, self._state.data_ptr(),
                    self._workspace.data_ptr(), self._workspace.numel(), self._stream()), "gbl_replay_prio_append")

    def set_priority(self, index: torch.Tensor, values: torch.Tensor) -> None:
        """The rows a batch drew get new priorities (``gbl_replay_prio_update``): ``index`` is the batch's "index" (int32 (batch, 2); only
        the slots are read, failed samples are skipped), ``values`` int32 (batch,).  A slot drawn more than once gets the largest of its
        values; the old priority is replaced."""
        self._need_priorities("set_priority")
        if index.dtype != torch.int32 or index.dim() != 2 or index.shape[1] != 2 or not index.is_contiguous() or index.device != self.device:
            raise ValueError("set_priority: index is a batch's 'index', int32 (batch, 2) on the buffer's device")
        values = values.to(torch.int32).contiguous()
        if values.shape != (index.shape[0],) or values.device != self.device:
            raise ValueError("set_priority: values must be (batch,) on the buffer's device")
        self._index_current = False
        with self._on_device():
            nat.check(self._lib.gbl_replay_prio_update(index.data_ptr(), values.data_ptr(), index.shape[0], self._prio.data_ptr(), self.capacity,
                                                       self._stream()), "gbl_replay_prio_update")

    def set_all_priority(self, values: torch.Tensor) -> None:
        """Priorities for the first ``len(values)`` slots, in slot order (a torch copy): the census of ``relabel(..., census=True)``
        mapped through a weight table, for instance."""
        self._need_priorities("set_all_priority")
        if values.dim() != 1 or values.shape[0] > self.capacity or values.is_floating_point():
            raise ValueError("set_all_priority: an integer tensor of at most capacity entries, in slot order")
        self._index_current = False
        self._prio[:values.shape[0]].copy_(values)

    def _rebuild_index(self) -> None:
        if not self._index_current:
            nat.check(self._lib.gbl_replay_prio_index(self._prio.data_ptr(), self.capacity, self._state.data_ptr(), self._index.data_ptr(),
                                                      self._index.numel() * 8, self._stream()), "gbl_replay_prio_index")
            self._index_current = True

    @staticmethod
    def importance_weights(batch: dict, beta: float = 1.0) -> torch.Tensor:
        """The importance weights of a prioritised batch, float32 (batch,) in torch: with p = priority / W the probability a row was drawn
        with and span the number of rows it was drawn from, (1 / (span p))^beta = (W / (span priority))^beta, divided by the largest of
        them; 0 for a failed sample."""
        w, total = batch["priority"].to(torch.float64), batch["prio_total"].to(torch.float64)
        raw = torch.where(w > 0, (total[0] / (total[1] * w.clamp(min=1))) ** float(beta), torch.zeros_like(w))
        return (raw / raw.max().clamp(min=torch.finfo(torch.float64).tiny)).to(torch.float32)

    def batch_weights(self, batch: dict, beta: float, out: torch.Tensor | None = None) -> torch.Tensor:
        """The importance weights of a prioritised batch dict on the device, float32 (batch,): one launch of ``gbl_replay_importance``
        (bit-defined; (smallest drawn priority / priority)^beta, 0 for a failed sample -- ``importance_weights`` within rounding), what
        ``GobbletTrainer.step(weights=...)`` takes.  ``out``: the tensor of an earlier call to write into."""
        self._need_priorities("batch_weights")
        if "priority" not in batch:
            raise ValueError("batch_weights: the dict of batch(..., prioritized=True)")
        prio = batch["priority"]
        beta = float(beta)
        if not 0.0 <= beta <= 1.0:
            raise ValueError("batch_weights: beta must be in [0, 1]")
        if out is None:
            out = torch.empty(prio.shape[0], dtype=torch.float32, device=self.device)
        elif out.shape != prio.shape or out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous():
            raise ValueError("out: the tensor of an earlier batch_weights call of this batch size on this buffer")
        with self._on_device():
            nat.check(self._lib.gbl_replay_importance(prio.data_ptr(), prio.shape[0], beta, out.data_ptr(), self._stream()),
                      "gbl_replay_importance")
        return out

    def batch(self, batch: int, symmetries="all", call: int = 0, seed: int = 0, recent: int | None = None, out: dict | None = None,
              prioritized: bool = False) -> dict:
        """``batch`` rows drawn exactly uniformly from the newest ``recent`` rows (None: from all the buffer holds), each under a random
        symmetry, one launch of ``gbl_replay_batch``: the keys of ``BatchedGobblet.training_batch`` -- "observation" (a buffer with
        observations), "action_mask", "visits", "z", "sym" -- with "index" int32 (batch, 2) = (slot, tag).  The draws are keyed by
        (``seed``, sample index, ``call``).  An empty buffer gives ``training_batch``'s failed samples (index (-1, -1), zero rows,
        z = ``nat.Z_OPEN``).  ``out``: a dict from an earlier call to write into.
        ``prioritized=True`` (a prioritised buffer): a row is drawn with probability priority / W instead, W the sum over the rows drawn
        from (``gbl_replay_batch_prio``; keyed alike on its own generator stream); the dict also holds "priority" int32 (batch,), the
        drawn rows' weights, and "prio_total" int64 (2,) = (W, the number of rows drawn from).  With W = 0 every sample is failed."""
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
        if prioritized:
            self._need_priorities("batch(prioritized=True)")
            spec.update(priority=((batch,), torch.int32), prio_total=((2,), torch.int64))
        if out is None:
            out = {k: torch.empty(shape, dtype=dtype, device=dev) for k, (shape, dtype) in spec.items()}
        elif set(out) != set(spec) or any(tuple(out[k].shape) != shape or out[k].dtype != dtype or out[k].device != dev
                                          or not out[k].is_contiguous() for k, (shape, dtype) in spec.items()):
            raise ValueError("out: the dict of an earlier batch call of this batch size on this buffer")
        with self._on_device():
            if prioritized:
                self._rebuild_index()
                nat.check(self._lib.gbl_replay_batch_prio(
                    nat.ptr(self._obs), self._visits.data_ptr(), self._meta.data_ptr(), self.capacity, self._state.data_ptr(),
                    self._prio.data_ptr(), self._index.data_ptr(), out["priority"].data_ptr(), out["prio_total"].data_ptr(), recent, batch,
                    BatchedGobblet.SYMMETRY_MASKS[symmetries], int(seed), 0, call, nat.ptr(out.get("observation")),
                    out["action_mask"].data_ptr(), out["visits"].data_ptr(), out["z"].data_ptr(), out["index"].data_ptr(),
                    out["sym"].data_ptr(), self._stream()), "gbl_replay_batch_prio")
                return out
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
        if nat.device(tb.device) != self.device:
            raise ValueError("relabel: the table lives on %s and the buffer on %s" % (tb.device, self.device))
        return tb._targets(self.size, self._obs.data_ptr(), nat.REPLAY_OBS_PITCH, self._meta.data_ptr(), nat.REPLAY_META_PITCH,
                           self._visits.data_ptr(), nat.REPLAY_VISITS_PITCH, self._meta.data_ptr() + nat.REPLAY_META_Z, nat.REPLAY_META_PITCH,
                           mode, count, census, None, allow_incomplete)

    def reanalyse(self, evaluator, iterations: int = 64, explore: int = 16, census: bool = False, prioritize: dict | None = None,
                  gumbel: dict | None = None, seed: int = 0, call: int = 0) -> dict:
        """Fresh search targets for the ring's live rows, in place: one launch of ``gbl_reanalyse`` over the ring's own arrays through
        their pitches -- the visits of every live row become the visit counts of ``evaluator``'s search (``GobbletEvaluator.reanalyse``
        has the rule) on the position the row's observation holds.  The live rows are ``relabel``'s: every slot once the ring has
        wrapped and the first ``total`` slots before; z, mover bytes, tags, masks, observations and padding are not touched.  Returns
        ``dict(drift=int32 (live rows,), census=int8 (live rows,) or None)`` in slot order.  ``prioritize=dict(floor=1, scale=1)`` (a
        prioritised buffer): every live row's priority becomes ``floor + scale * max(drift, 0)`` on the device (``set_priority``'s
        path), so rows whose targets moved furthest are drawn first.  Reads ``total`` from the device, nothing else.
        ``gumbel=dict(considered=16, noise=True, visit_offset=50, scale=23)``: one launch of ``gbl_reanalyse_gumbel`` instead -- the
        rows become the Gumbel root search's target rows (``GobbletEvaluator.reanalyse`` has the rule), the kind of row a ring filled by
        ``collect(search=dict(gumbel=...))`` holds; the noise of a row is keyed by (``seed``, its slot, ``call``).  ``prioritize`` works
        unchanged on the new drift."""
        if self._obs is None:
            raise ValueError("reanalyse needs a buffer with observations")
        rule = None if gumbel is None else gumbel_args(gumbel)
        if nat.device(evaluator.device) != self.device:
            raise ValueError("reanalyse: the evaluator lives on %s and the buffer on %s" % (evaluator.device, self.device))
        if prioritize is not None:
            self._need_priorities("reanalyse(prioritize=...)")
            if set(prioritize) - {"floor", "scale"}:
                raise ValueError("reanalyse: prioritize=dict(floor=1, scale=1)")
            floor, scale = int(prioritize.get("floor", 1)), int(prioritize.get("scale", 1))
            if floor < 0 or scale < 0 or floor + scale * 1024 >= 1 << 31:
                raise ValueError("reanalyse: floor and scale must be >= 0 and floor + 1024 * scale must fit an int32")
        live = self.size
        drift, tally = evaluator._reanalyse(live, self._obs.data_ptr(), nat.REPLAY_OBS_PITCH, self._meta.data_ptr(), nat.REPLAY_META_PITCH,
                                            self._visits.data_ptr(), self._visits.data_ptr(), nat.REPLAY_VISITS_PITCH,
                                            self._meta.data_ptr() + nat.REPLAY_META_Z, nat.REPLAY_META_PITCH, iterations, explore, census,
                                            None, rule, seed, 0, call)
        if prioritize is not None and live:
            slots = torch.arange(live, dtype=torch.int32, device=self.device)
            self.set_priority(torch.stack([slots, torch.zeros_like(slots)], dim=1).contiguous(), floor + scale * drift.clamp(min=0))
        return dict(drift=drift, census=tally)

    def fit(self, trainer, steps: int, batch: int = 1024, symmetries="all", first_call: int = 0, recent: int | None = None,
            seed: int = 0, targets=None, prioritized: bool = False, beta=None, priority: dict | None = None,
            reanalyse: dict | None = None) -> torch.Tensor:
        """``steps`` Adam steps of ``trainer`` (a ``GobbletTrainer`` on this buffer's device): step i draws ``batch(batch, symmetries,
        call=first_call + i, recent=recent)`` into one reused buffer and hands it to ``trainer.step``; nothing crosses to the host.
        ``targets``: a ``Tablebase`` on this device -- every drawn batch goes through ``targets.targets`` first (one more launch per
        step: the fit learns from the exact labels).  Returns the steps' statistics, float32 (steps, 4) on the device, as
        ``BatchedGobblet.fit`` does.  ``prioritized``: the batches are ``batch(..., prioritized=True)``'s.
        ``beta`` and ``priority`` (both need ``prioritized=True``) close the loop of prioritised replay.  ``beta``: a float, or a
        (start, end) pair annealed linearly over the steps (computed on the host in double) -- every batch's rows count with their
        ``batch_weights(buf, beta)`` in the step.  ``priority``: ``dict(scale=, floor=1, cap=)`` -- after every step the drawn rows get
        ``trainer.last_priority`` (``set_priority``), so the next draw rebuilds the index from the trainer's own losses.  A full step
        is then nine launches on one stream, and the host reads nothing: index build 2, draw 1, weights 1, step 2, the trainer's
        running maximum 1, priority update 2 (``targets`` adds its one, before the weights).
        ``reanalyse``: ``dict(evaluator=, iterations=64, explore=16)`` with a ``GobbletEvaluator`` on this device -- every drawn batch goes
        through ``evaluator.reanalyse`` first (one more launch per step, ``gbl_reanalyse``, in ``targets``' place: the two exclude each
        other): the step learns from the visit counts of that network's search instead of the stored ones, z stays the game's outcome.
        It composes with ``prioritized``, ``beta`` and ``priority``.  With ``gumbel=dict(considered=16, noise=True, visit_offset=50,
        scale=23)`` in the dict (and ``seed=0``) the launch is ``gbl_reanalyse_gumbel``'s: the step learns from the Gumbel root search's
        target rows, made for ``iterations=16`` or fewer; step i's noise is keyed by (seed, the row's place in the batch,
        ``first_call + i``), so every step's noise is fresh.  The drawn row is a symmetric image of the stored one, which is sound
        because the search commutes with the symmetries -- with ``gbl_symmetry_apply``'s caveat: check_for_winner's last-line-decides
        rule is not symmetric on boards where a move leaves lines of both colours, so under the squares' symmetries a search that
        reaches such a board may differ from the image of the stored row's search (``symmetries=None`` avoids it)."""
        if nat.device(trainer.device) != self.device:
            raise ValueError("fit: the trainer lives on %s and the buffer on %s" % (trainer.device, self.device))
        if (beta is not None or priority is not None) and not prioritized:
            raise ValueError("fit: beta= and priority= need prioritized=True")
        if reanalyse is not None:
            if targets is not None:
                raise ValueError("fit: targets= and reanalyse= exclude each other")
            unknown = set(reanalyse) - {"evaluator", "iterations", "explore", "gumbel", "seed"}
            if unknown or "evaluator" not in reanalyse or ("seed" in reanalyse and reanalyse.get("gumbel") is None):
                raise ValueError("fit: reanalyse=dict(evaluator=, iterations=64, explore=16, gumbel=None, seed=0) (seed goes with gumbel)")
            rule = None if reanalyse.get("gumbel") is None else gumbel_args(reanalyse["gumbel"])
            if nat.device(reanalyse["evaluator"].device) != self.device:
                raise ValueError("fit: the evaluator lives on %s and the buffer on %s" % (reanalyse["evaluator"].device, self.device))
            fresh = torch.zeros((int(batch), nat.ACTIONS), dtype=torch.int16, device=self.device)  # (reused: a skipped row counts for nothing)

            def relabelled(rows, i):
                return reanalyse["evaluator"].reanalyse(rows, reanalyse.get("iterations", 64), reanalyse.get("explore", 16), out=fresh, gumbel=rule,
                                                        seed=reanalyse.get("seed", 0), call=int(first_call) + i)
        elif targets is not None:
            def relabelled(rows, i):
                return targets.targets(dict(rows))
        else:
            def relabelled(rows, i):
                return rows
        buf, stats = None, []
        if beta is not None or priority is not None:
            steps = int(steps)
            ends = (float(beta[0]), float(beta[1])) if isinstance(beta, (tuple, list)) else None
            weights = None
            for i in range(steps):
                buf = self.batch(batch, symmetries=symmetries, call=int(first_call) + i, seed=seed, recent=recent, out=buf, prioritized=True)
                rows = relabelled(buf, i)
                if beta is not None:
                    b = float(beta) if ends is None else ends[0] + (ends[1] - ends[0]) * (i / (steps - 1) if steps > 1 else 0.0)
                    weights = self.batch_weights(buf, b, out=weights)
                stats.append(trainer.step(rows, weights=weights, priority=priority))
                if priority is not None:
                    self.set_priority(buf["index"], trainer.last_priority)
            return torch.stack(stats) if stats else torch.zeros((0, 4), dtype=torch.float32, device=self.device)
        for i in range(int(steps)):
            buf = self.batch(batch, symmetries=symmetries, call=int(first_call) + i, seed=seed, recent=recent, out=buf, prioritized=prioritized)
            stats.append(trainer.step(relabelled(buf, i)))
        return torch.stack(stats) if stats else torch.zeros((0, 4), dtype=torch.float32, device=self.device)

    def state_dict(self) -> dict:
        if self.prioritized:
            return {**self._ring_state_dict(), "priority": self._prio.clone()}
        return self._ring_state_dict()

    def _ring_state_dict(self) -> dict:
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
        if self.prioritized:
            if "priority" not in state:
                raise ValueError("load_state_dict: the state is of a buffer without priorities")
            self._prio.copy_(state["priority"])
            self._index_current = False
