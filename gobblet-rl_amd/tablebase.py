"""The exact tablebase: ``Tablebase`` owns one byte per position of an inventory on one device (include/gobblet_hip.h, "Exact
tablebase") -- 2 881 473 967 bytes for the game's own inventory (2, 2, 2) -- builds it by retrograde sweeps (``gbl_tb_sweep``) and
answers from it (``gbl_tb_probe``): the true result of every action at any depth, one gather per action.  ``TablebaseGobbletPolicy``
plays from it with ``SolverGobbletPolicy``'s surface.  Smaller inventories are the same rules with fewer pieces and build in
milliseconds; ``device="cpu"`` is the host flavour of the ABI, and a table saved on one device can be loaded and probed on another."""
from __future__ import annotations

import json
from typing import Any

import numpy as np
import torch

from . import _native as nat
from ._policy_base import _OnDevice, _SearchPolicy

MAGIC = b"GBLTB001"
HEADER_BYTES = 4096  # the magic, then a JSON object padded with spaces (127 ten-digit counts fit); the table's bytes follow


class Tablebase(_OnDevice):
    def __init__(self, inventory=(2, 2, 2), device="cuda:0") -> None:
        """An empty table (no sweep done) of ``inventory`` = each player's number of pieces of size 0, 1, 2 (each 0 .. 2)."""
        inventory = tuple(int(c) for c in inventory)
        if len(inventory) != 3 or not all(0 <= c <= 2 for c in inventory):
            raise ValueError("inventory: three piece counts, each in [0, 2]")
        self.inventory, self.device = inventory, nat.device(device)
        self._lib = nat.lib_for(self.device)
        self._inv = (nat.C.c_int32 * 3)(*inventory)
        layout = (nat.C.c_int64 * 5)()
        nat.check(nat.lib().gbl_tb_layout(self._inv, layout), "gbl_tb_layout")  # (one function for both flavours: it launches nothing)
        self.positions, self.levels = int(layout[0]), tuple(int(x) for x in layout[1:4])
        self._aux = torch.zeros(int(layout[4]), dtype=torch.uint8, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_tb_prepare(self._inv, self._aux.data_ptr(), self._stream()), "gbl_tb_prepare")
        self.table = torch.zeros(self.positions, dtype=torch.int8, device=self.device)
        self._decided = torch.zeros(1, dtype=torch.int64, device=self.device)  # (the ABI's uint64)
        self.sweeps, self.complete, self.decided = 0, False, []  # sweeps done (sweep 0 counts), and what each wrote non-zero

    def sweep(self, k: int, first: int = 0, count: int | None = None, out: torch.Tensor | None = None, table: torch.Tensor | None = None) -> None:
        """One launch of ``gbl_tb_sweep`` on this table: sweep ``k`` over [first, first + count), in place unless ``out`` (int8, count
        bytes) is given; the bytes written non-zero are added to the device counter.  Waits for nothing."""
        count = self.positions - first if count is None else count
        table = self.table if table is None else table
        dst = table.data_ptr() + first if out is None else out.data_ptr()
        with self._on_device():
            nat.check(self._lib.gbl_tb_sweep(self._inv, self._aux.data_ptr(), table.data_ptr(), dst, int(first), int(count), int(k),
                                             self._decided.data_ptr(), self._stream()), "gbl_tb_sweep")

    def build(self, max_sweeps: int | None = None, slice_positions: int | None = None) -> list:
        """Sweeps from where the table stands until one decides nothing (``complete`` becomes True) or ``max_sweeps`` sweeps have been
        done in this call; every sweep in place, cut into launches of ``slice_positions`` positions (None: one launch).  Reads the
        device counter once per sweep.  Returns ``decided``: the bytes each sweep wrote non-zero, sweep 0 first.  A build whose next
        sweep would be 127 raises instead of wrapping the byte."""
        step = self.positions if slice_positions is None else int(slice_positions)
        if step < 1:
            raise ValueError("build: slice_positions must be positive")
        done = 0
        while not self.complete and (max_sweeps is None or done < max_sweeps):
            k = self.sweeps
            if k > nat.TB_MAX_SWEEP:
                raise nat.GobbletHipError("build: sweep %d would not fit the byte (GBL_TB_MAX_SWEEP = %d)" % (k, nat.TB_MAX_SWEEP))
            self._decided.zero_()
            for first in range(0, self.positions, step):
                self.sweep(k, first, min(step, self.positions - first))
            wrote = int(self._decided[0])
            self.decided.append(wrote)
            self.sweeps, done = k + 1, done + 1
            self.complete = k > 0 and wrote == 0
        return list(self.decided)

    # ---- questions ---------------------------------------------------------------------------------------------------------------
    def probe(self, squares, to_move, mask=None) -> dict:
        """``gbl_solve``'s three outputs with no depth bound, read from the table: "outcome" int8 (N, 54), "value" int8 (N,), "action"
        int32 (N,) (``BatchedGobblet.solve``'s dict).  On a table that is not complete, 0 reads "not proven by the sweeps done"."""
        state, to_move, mask = self._inputs(squares, to_move, mask)
        n = state.shape[0]
        out = {"outcome": torch.empty((n, nat.ACTIONS), dtype=torch.int8, device=self.device),
               "value": torch.empty(n, dtype=torch.int8, device=self.device), "action": torch.empty(n, dtype=torch.int32, device=self.device)}
        with self._on_device():
            nat.check(self._lib.gbl_tb_probe(self._inv, self._aux.data_ptr(), self.table.data_ptr(), state.data_ptr(), to_move.data_ptr(),
                                             nat.ptr(mask), out["outcome"].data_ptr(), out["value"].data_ptr(), out["action"].data_ptr(), n,
                                             self._stream()), "gbl_tb_probe")
        return out

    def index(self, squares, to_move) -> torch.Tensor:
        """int64 (N,): each board's index as its side to move sees it; -1 where the board is no state of the inventory."""
        state, to_move, _ = self._inputs(squares, to_move, None)
        out = torch.empty(state.shape[0], dtype=torch.int64, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_tb_index(self._inv, self._aux.data_ptr(), state.data_ptr(), to_move.data_ptr(), out.data_ptr(),
                                             state.shape[0], self._stream()), "gbl_tb_index")
        return out

    def position(self, indices) -> torch.Tensor:
        """int8 (N, 27): the position of each index as a contract state with player_1 to move."""
        idx = torch.as_tensor(indices).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        out = torch.empty((idx.shape[0], nat.CELLS), dtype=torch.int8, device=self.device)
        with self._on_device():
            nat.check(self._lib.gbl_tb_position(self._inv, self._aux.data_ptr(), idx.data_ptr(), out.data_ptr(), idx.shape[0], self._stream()),
                      "gbl_tb_position")
        return out

    def value(self, indices) -> torch.Tensor:
        """int8 (N,): the table's bytes at ``indices`` (``nat.TB_TERMINAL`` where the position already holds a line)."""
        return self.table[torch.as_tensor(indices).to(device=self.device, dtype=torch.int64).reshape(-1)]

    # ---- exact training targets -------------------------------------------------------------------------------------------------
    def _targets(self, n, obs, obs_pitch, mask, mask_pitch, visits, visits_pitch, z, z_pitch, mode, count, census, value, allow_incomplete):
        """One launch of ``gbl_tb_targets`` in place on ``n`` pitched rows (data pointers); returns the census tensor or None."""
        if mode not in nat.TB_TARGET_MODES:
            raise ValueError("mode: 'result' or 'shortest'")
        if not 1 <= int(count) <= nat.TB_TARGET_MAX_COUNT:
            raise ValueError("count must be in [1, %d]" % nat.TB_TARGET_MAX_COUNT)
        if not self.complete and not allow_incomplete:
            raise ValueError("the table is not complete: a 0 would read 'not proven yet' (allow_incomplete=True to label with it anyway)")
        tally = torch.empty(n, dtype=torch.int8, device=self.device) if census else None
        with self._on_device():
            nat.check(self._lib.gbl_tb_targets(self._inv, self._aux.data_ptr(), self.table.data_ptr(), obs, obs_pitch, mask, mask_pitch, visits,
                                               visits, visits_pitch, z, z, z_pitch, nat.TB_TARGET_MODES[mode], int(count), nat.ptr(value), None,
                                               nat.ptr(tally), n, self._stream()), "gbl_tb_targets")
        return tally

    def targets(self, batch: dict, mode: str = "result", count: int = 1, census: bool = False, allow_incomplete: bool = False) -> dict:
        """Exact targets for the dict ``BatchedGobblet.training_batch`` / ``ReplayBuffer.batch`` return, one launch of ``gbl_tb_targets``:
        "visits" and "z" are overwritten IN PLACE -- ``count`` on every candidate that keeps the true result (``mode`` "result") or
        that is a shortest win, a draw or a longest loss ("shortest"), z = the true sign; a failed sample stays as it is, a row the
        table cannot label gets zero visits and z = ``nat.Z_OPEN``.  Adds "tb_value" int8 (N,) and, with ``census``, "census" int8 (N,)
        (include/gobblet_hip.h, "Tablebase targets": bit 0 the old visits' argmax kept the result, bit 1 the old z was the true sign,
        bit 2 there were no old visits; -1 for a row without a label).  Returns the dict."""
        if "observation" not in batch:
            raise ValueError("targets needs the 'observation' entry: a window or a buffer with observations")
        obs, mask, visits, z = batch["observation"], batch.get("action_mask"), batch["visits"], batch["z"]
        n = int(z.shape[0])
        spec = (("observation", obs, (n, nat.OBS_BYTES), torch.int8), ("action_mask", mask, (n, nat.ACTIONS), torch.int8),
                ("visits", visits, (n, nat.ACTIONS), torch.int16), ("z", z, (n,), torch.int8))
        for name, t, shape, dtype in spec:
            if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or t.device != self.device or not t.is_contiguous()):
                raise ValueError(f"targets: {name} must be a contiguous {dtype} tensor of shape {shape} on {self.device}")
        value = torch.empty(n, dtype=torch.int8, device=self.device)
        tally = self._targets(n, obs.data_ptr(), nat.OBS_BYTES, nat.ptr(mask), nat.ACTIONS, visits.data_ptr(), nat.ACTIONS, z.data_ptr(), 1,
                              mode, count, census, value, allow_incomplete)
        batch["tb_value"] = value
        if census:
            batch["census"] = tally
        return batch

    # ---- the verdict of a collected window -----------------------------------------------------------------------------------------
    REGRET_CLASSES = ("kept", "win_to_draw", "win_to_loss", "draw_to_loss", "no_verdict")

    def judge(self, traj: dict, boards: int | None = None) -> dict:
        """What a window collected with ``search=dict(tablebase=..., judge=True)`` did with the truth (torch only, on the trajectory's
        device).  Adds to ``traj``: "z_exact" int8 per cell, the sign of "tb_value" (``nat.Z_OPEN`` where the table holds no verdict:
        the outcome row is all ``nat.SOLVE_NONE``), and "regret" int8 per cell: 0 the played action kept the result, 1 a win became a
        draw, 2 a win became a loss, 3 a draw became a loss, -1 no verdict (also an action that was no candidate).  Returns the counts
        of each class per side: ``{"player_1": {"kept": ..., "win_to_draw": ..., "win_to_loss": ..., "draw_to_loss": ...,
        "no_verdict": ...}, "player_2": {...}}``, by "mover".  ``boards``: in the "tile" layout the number of boards of the window
        (cells past it in the last tile were never written and are not counted)."""
        for k in ("tb_outcomes", "tb_value", "tb_played", "mover"):
            if k not in traj:
                raise ValueError("judge needs the %r entry: buffers from trajectory_buffers(tablebase_outputs=True)" % k)
        value, played, mover = traj["tb_value"], traj["tb_played"], traj["mover"]
        none = (traj["tb_outcomes"] == nat.SOLVE_NONE).all(-1)
        sv, sp = torch.sign(value.to(torch.int16)), torch.sign(played.to(torch.int16))
        regret = torch.zeros_like(value)
        regret[(sv == 1) & (sp == 0)] = 1
        regret[(sv == 1) & (sp == -1)] = 2
        regret[(sv == 0) & (sp == -1)] = 3
        regret[none | (played == nat.SOLVE_NONE)] = -1
        traj["z_exact"] = torch.where(none, torch.full_like(value, nat.Z_OPEN), sv.to(torch.int8))
        traj["regret"] = regret
        counted = torch.ones_like(none)
        if boards is not None and traj.get("_layout") == "tile":
            tiles, plies = value.shape[0], value.shape[1]
            counted = (torch.arange(tiles * 64, device=value.device).reshape(tiles, 1, 64) < int(boards)).expand(tiles, plies, 64)
        out = {}
        for m, name in enumerate(("player_1", "player_2")):
            mine = counted & (mover == m)
            out[name] = {c: int((mine & (regret == (k if k < 4 else -1))).sum()) for k, c in enumerate(self.REGRET_CLASSES)}
        return out

    # ---- files: a header and the raw bytes (never part of the repository: the full table is 2.9 GB) -------------------------------
    def save(self, path) -> None:
        head = json.dumps({"inventory": list(self.inventory), "positions": self.positions, "sweeps": self.sweeps, "complete": self.complete,
                           "decided": self.decided}).encode()
        if len(MAGIC) + len(head) > HEADER_BYTES:
            raise ValueError("save: the header does not fit")
        with open(path, "wb") as f:
            f.write((MAGIC + head).ljust(HEADER_BYTES, b" "))
            step = 1 << 28
            for first in range(0, self.positions, step):  # (in pieces: no second copy of the table on the host)
                f.write(self.table[first:first + step].cpu().numpy().tobytes())

    @classmethod
    def load(cls, path, device="cuda:0") -> "Tablebase":
        with open(path, "rb") as f:
            raw = f.read(HEADER_BYTES)
            if len(raw) != HEADER_BYTES or raw[:len(MAGIC)] != MAGIC:
                raise ValueError("load: %s is no tablebase file" % path)
            head = json.loads(raw[len(MAGIC):].decode())
            tb = cls(tuple(head["inventory"]), device)
            if tb.positions != int(head["positions"]):
                raise ValueError("load: the file's size does not match its inventory")
            step = 1 << 28
            for first in range(0, tb.positions, step):
                part = np.frombuffer(f.read(min(step, tb.positions - first)), np.int8)
                if len(part) != min(step, tb.positions - first):
                    raise ValueError("load: %s is truncated" % path)
                tb.table[first:first + len(part)] = torch.from_numpy(part.copy()).to(tb.device)
        tb.sweeps, tb.complete, tb.decided = int(head["sweeps"]), bool(head["complete"]), [int(x) for x in head["decided"]]
        return tb


class TablebaseGobbletPolicy(_SearchPolicy):
    def __init__(self, tb: Tablebase, fallback=None, **kwargs: Any) -> None:
        """Plays from ``tb``: the shortest win, else an action whose result is 0 (a draw on a complete table), else the longest loss.
        fallback: a policy of this package on the table's device that decides among the 0 actions of a root whose value is 0 (the
        table by itself plays the lowest of them)."""
        self.tb, self.device, self._lib = tb, tb.device, tb._lib
        if fallback is not None and nat.device(fallback.device) != self.device:
            raise ValueError("the fallback policy must live on the table's device")
        self.fallback = fallback
        self.last_outcomes = self.last_value = self.last_action = None

    def _run(self, state, to_move, mask) -> torch.Tensor:
        out = self.tb.probe(state, to_move, mask)
        self.last_outcomes, self.last_value, self.last_action = out["outcome"], out["value"], out["action"]
        return out["action"]

    def compute_actions_from_state(self, state, to_move, mask=None) -> torch.Tensor:
        """int32 (N,), -1 where a board has no candidate; with a ``fallback``, the boards of value 0 are its decision among their 0
        actions (``SolverGobbletPolicy``'s rule, with the table's verdict in place of the bounded one)."""
        state, to_move, mask = self._inputs(state, to_move, mask)
        act = self._run(state, to_move, mask)
        if self.fallback is None:
            return act
        open_ = (self.last_outcomes == 0).to(torch.int8)
        undecided = open_.any(1) & (self.last_value == 0)
        if bool(undecided.any()):
            rows = torch.nonzero(undecided).reshape(-1)
            theirs = self.fallback.compute_actions_from_state(state[rows], to_move[rows], open_[rows])
            act = act.clone()
            act[rows] = theirs.to(device=self.device, dtype=torch.int32)
        return act

    def outcomes(self, state, to_move, mask=None) -> torch.Tensor:
        """int8 (N, 54): the table's result of every candidate action, ``nat.SOLVE_NONE`` elsewhere."""
        self._run(*self._inputs(state, to_move, mask))
        return self.last_outcomes
