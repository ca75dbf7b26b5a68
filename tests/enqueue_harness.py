"""One raw C-ABI call of every compute entry point that has no graph-capture test of its own, on pre-allocated tensors at the smallest
shapes (65 boards or rows, hidden 64, 8 iterations, inventory (1, 1, 1)): ``TABLE`` = (name, make_args, outputs).  ``world(dev)``
builds the tensors with the package itself, the same bits on either flavour; ``make_args(w, stream)`` is the argument list in the
ABI's order with ``stream`` last; ``outputs`` names the tensors the call changes (pure outputs start as canaries) -- those and no other.
tests/test_host_threads.py runs the table on the host flavour (the reference); tests/test_gpu_devices_threads.py captures every
call on a side stream and replays it.  A plain module: nothing here is collected."""
import ctypes as C

import torch

import gobblet_rl_amd as G
from tests import host_contract_harness as H

nat = G._native
N, T, B, HIDDEN, ITER, CAP = 65, 4, 65, 64, 8, 100
CANARY = 90


class World:
    """``t``: the tensors by name (views of fresh allocations on one device); ``c``: host-side values and the objects that own
    memory the calls read."""

    def __init__(self, dev):
        self.dev, self.t, self.c = dev, {}, {}

    def p(self, name):
        return None if name is None else self.t[name].data_ptr()

    def canary(self, name, shape, dtype):
        self.t[name] = torch.full(tuple(shape), CANARY, dtype=dtype).to(self.dev)

    def snapshot(self):
        return {k: v.clone() for k, v in self.t.items()}

    def restore(self, snap):
        for k, v in self.t.items():
            v.copy_(snap[k])


def world(dev) -> World:
    w = World(dev)
    t, c = w.t, w.c
    ev = H.evaluator(dev)
    c["ev_obj"], c["ev"] = ev, ev.as_struct()
    env = G.BatchedGobblet(N, dev, auto_reset=True, seed=5, track_turn=True)
    env.rollout(20)
    tr = env.collect(T, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=ITER, sample_plies=2), out="fresh")
    env.outcome_targets(tr)
    c["ply_stride"], c["tile_stride"] = tr["_ply_stride"], tr["_tile_stride"]
    for k in ("observation", "action_mask", "visits", "z", "done", "mover", "rewards"):
        t["traj." + k] = tr["_full"][k]
    w.canary("traj.z_out", t["traj.z"].shape, torch.int8)
    w.canary("traj.plies_left_out", t["traj.z"].shape, torch.int16)
    # the boards after the window, what one more ply needs, and a canary for everything a ply writes
    t["state"], t["to_move"], t["done"], t["turn"] = env.squares.clone(), env.to_move.clone(), env.done.clone(), env.turn.clone()
    t["mask"], t["obs"], t["actions"] = env.action_mask.clone(), env.observation.clone(), env.sample_actions().clone()
    t["hist"] = torch.full((N, 2, 3), -1, dtype=torch.int8).to(dev)
    t["counters"] = torch.zeros((nat.COUNTER_STRIPES, nat.COUNTER_STRIDE), dtype=torch.int64).to(dev)
    for name, tail, dtype in (("winner", (), torch.int8), ("reward", (2,), torch.int8), ("mask", (nat.ACTIONS,), torch.int8),
                              ("obs", (3, 3, 13), torch.int8), ("actions", (), torch.int32), ("done", (), torch.int8),
                              ("to_move", (), torch.int8), ("status", (), torch.int8), ("next", (), torch.int32), ("flat", (9,), torch.int8),
                              ("covered", (nat.CELLS,), torch.int8), ("flags", (), torch.int8), ("legal", (), torch.int8),
                              ("record", (nat.REC_BYTES,), torch.int8), ("state", (nat.CELLS,), torch.int8), ("chosen", (), torch.int32),
                              ("cand", (nat.ACTIONS,), torch.int8), ("fallback", (), torch.int8), ("wins", (), torch.int32),
                              ("losses", (), torch.int32), ("plies", (), torch.int32), ("nodes", (), torch.int32), ("root_value", (), torch.int32),
                              ("visits54", (nat.ACTIONS,), torch.int32), ("wins54", (nat.ACTIONS,), torch.int32),
                              ("losses54", (nat.ACTIONS,), torch.int32), ("priors", (nat.ACTIONS,), torch.uint8),
                              ("mixed", (nat.ACTIONS,), torch.uint8), ("target", (nat.ACTIONS,), torch.uint8), ("gumbel", (nat.ACTIONS,), torch.int16),
                              ("logits", (56,), torch.int32), ("value", (), torch.int32), ("visits16", (nat.ACTIONS,), torch.int16),
                              ("actions_img", (), torch.int32), ("outcome", (nat.ACTIONS,), torch.int8), ("value8", (), torch.int8),
                              ("index64", (), torch.int64)):
        w.canary("out." + name, (N,) + tail, dtype)
    # trajectory buffers of the environment's own making for the collect entry points, every array a canary
    bufs = env.trajectory_buffers(T, placement="any", policy_outputs=True, candidates=True)
    assert (bufs["_ply_stride"], bufs["_tile_stride"]) == (c["ply_stride"], c["tile_stride"])
    for k, v in bufs["_full"].items():
        v.fill_(CANARY)
        t["win." + k] = v
    # drawn rows: what the trainer, the table's targets and the reanalysis read
    rows = env.training_batch(tr, B, call=0)
    for k in ("observation", "action_mask", "visits", "z"):
        t["rows." + k] = rows[k]
    for k, v in rows.items():
        w.canary("draw." + k, v.shape, v.dtype)
    w.canary("draw.priority", (B,), torch.int32)
    w.canary("draw.prio_total", (2,), torch.int64)
    t["sym"] = (torch.arange(N) * 37 % nat.SYMMETRIES).to(torch.int16).to(dev)
    w.canary("rows.visits_out", (B, nat.ACTIONS), torch.int16)
    w.canary("rows.z_out", (B,), torch.int8)
    w.canary("rows.drift", (B,), torch.int32)
    w.canary("rows.tally", (B,), torch.int8)
    w.canary("rows.root_value", (B,), torch.int32)
    w.canary("rows.gumbel", (B, nat.ACTIONS), torch.int16)
    w.canary("rows.tb_value", (B,), torch.int8)
    # the ring of a prioritised buffer that holds the window once, its index current
    buf = G.ReplayBuffer(CAP, dev, prioritized=True)
    buf.append(env, tr, tag=1, priority=3)
    drawn = buf.batch(B, call=1, seed=3, prioritized=True)
    c["buf"] = buf
    t["ring.obs"], t["ring.visits"], t["ring.meta"], t["ring.state"] = buf._obs, buf._visits, buf._meta, buf._state
    t["ring.prio"], t["ring.index"], t["ws.ring"] = buf._prio, buf._index, buf._workspace
    w.canary("ring.index_out", buf._index.shape, torch.int64)
    t["drawn.index"], t["drawn.priority"] = drawn["index"], drawn["priority"]
    t["drawn.values"] = (torch.arange(B) % 7).to(torch.int32).to(dev)
    t["cells.prio"] = (torch.arange(t["traj.z"].numel()).reshape(t["traj.z"].shape) % 5).to(torch.int32).to(dev)
    w.canary("out.weights", (B,), torch.float32)
    # the (1, 1, 1) table, complete, and one that has done sweep 0 only
    tb, part = G.Tablebase((1, 1, 1), dev), G.Tablebase((1, 1, 1), dev)
    tb.build()
    part.build(max_sweeps=1)
    c["tb"], c["inv"], c["positions"], c["sweep"] = tb, tb._inv, tb.positions, part.sweeps
    t["tb.aux"], t["tb.table"], t["tb.part"] = tb._aux, tb.table, part.table
    t["tb.decided"] = torch.zeros(1, dtype=torch.int64).to(dev)
    w.canary("tb.aux_out", t["tb.aux"].shape, torch.uint8)
    t["tb.sweep_out"] = part.table.clone()  # (the range after sweep 0: what sweep 1 takes in `out`)
    t["small.index"] = (torch.arange(N, dtype=torch.int64) * (tb.positions // N)).to(dev)
    t["small.state"] = tb.position(t["small.index"])
    t["small.to_move"] = (torch.arange(N) % 2).to(torch.int8).to(dev)
    # the float network, Adam's moments and the step's buffers
    net = G.GobbletTrainer(hidden=HIDDEN, device=dev, seed=3)
    t["net.params"], t["net.m"], t["net.v"], t["net.grad"] = net.params, net.m, net.v, net.last_grad
    w.canary("net.stats", (4,), torch.float32)
    w.canary("net.row_loss", (B, 2), torch.float32)
    w.canary("net.priority", (B,), torch.int32)
    t["net.weights"] = torch.linspace(0.5, 1.5, B, dtype=torch.float32).to(dev)
    t["ws.net"] = torch.zeros(nat.lib().gbl_train_workspace_bytes(B, HIDDEN), dtype=torch.uint8).to(dev)
    c["hyper"] = nat.TrainHyper(net.lr, net.betas[0], net.betas[1], net.eps, net.weight_decay, net.value_reg, 1.0 - net.betas[0], 1.0 - net.betas[1])
    return w


def _ev(w):
    return C.addressof(w.c["ev"])


def _strides(w):
    return N, w.c["ply_stride"], w.c["tile_stride"]


def _table(w, table="tb.table"):
    return w.c["inv"], w.p("tb.aux"), w.p(table)


def _rows(w):  # (obs, pitch, mask, pitch) of the drawn rows
    return w.p("rows.observation"), nat.OBS_BYTES, w.p("rows.action_mask"), nat.ACTIONS


def _step_head(w):
    return (w.p("state"), w.p("to_move"), w.p("done"), w.p("actions"), w.p("out.winner"), w.p("out.reward"), w.p("out.mask"), w.p("out.obs"),
            w.p("turn"))


def _win(w, *keys):
    return tuple(w.p("win." + k) for k in keys)


_WIN = ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation")
_WIN_OUT = tuple("win." + k for k in _WIN)
_BOARDS = ("state", "to_move", "done")
_PLY_OUT = ("turn", "out.winner", "out.reward", "out.mask", "out.obs")  # (what one ply writes beside the boards)
_DRAW = ("observation", "action_mask", "visits", "z", "index", "sym")
_DRAW_OUT = tuple("draw." + k for k in _DRAW)
_TRAIN = ("rows.observation", "rows.action_mask", "rows.visits", "rows.z")
_SEARCH_OUT = ("out.visits54", "out.wins54", "out.losses54", "out.actions", "out.nodes")

# (name, make_args(w, stream), the tensors the call changes)
TABLE = [
    # ---- the multi-launch entry points, the searches and the row kernels ----
    ("gbl_train_step", lambda w, s: (*(w.p(k) for k in _TRAIN), B, HIDDEN, w.p("net.params"), w.p("net.m"), w.p("net.v"),
                                     C.addressof(w.c["hyper"]), w.p("net.grad"), w.p("net.stats"), w.p("ws.net"), w.t["ws.net"].numel(), s),
     ("net.params", "net.m", "net.v", "net.grad", "net.stats")),
    ("gbl_train_step_weighted", lambda w, s: (*(w.p(k) for k in _TRAIN), B, HIDDEN, w.p("net.params"), w.p("net.m"), w.p("net.v"),
                                              C.addressof(w.c["hyper"]), w.p("net.weights"), w.p("net.row_loss"), w.p("net.priority"), 16.0, 1, 1000,
                                              w.p("net.grad"), w.p("net.stats"), w.p("ws.net"), w.t["ws.net"].numel(), s),
     ("net.params", "net.m", "net.v", "net.grad", "net.stats", "net.row_loss", "net.priority")),
    ("gbl_replay_append", lambda w, s: (w.p("traj.observation"), w.p("traj.action_mask"), w.p("traj.visits"), w.p("traj.z"), w.p("traj.done"),
                                        w.p("traj.mover"), N, T, w.c["ply_stride"], w.c["tile_stride"], 2, w.p("ring.obs"), w.p("ring.visits"),
                                        w.p("ring.meta"), CAP, w.p("ring.state"), w.p("ws.ring"), w.t["ws.ring"].numel(), s),
     ("ring.obs", "ring.visits", "ring.meta", "ring.state")),
    ("gbl_replay_batch", lambda w, s: (w.p("ring.obs"), w.p("ring.visits"), w.p("ring.meta"), CAP, w.p("ring.state"), 0, B, nat.SYMMETRIES - 1, 9, 0, 2,
                                       *(w.p(k) for k in _DRAW_OUT), s), _DRAW_OUT),
    ("gbl_replay_prio_append", lambda w, s: (w.p("traj.visits"), w.p("traj.z"), w.p("traj.done"), w.p("cells.prio"), 0, N, T, w.c["ply_stride"],
                                             w.c["tile_stride"], w.p("ring.prio"), CAP, w.p("ring.state"), w.p("ws.ring"), w.t["ws.ring"].numel(), s),
     ("ring.prio",)),
    ("gbl_replay_prio_update", lambda w, s: (w.p("drawn.index"), w.p("drawn.values"), B, w.p("ring.prio"), CAP, s), ("ring.prio",)),
    ("gbl_replay_prio_index", lambda w, s: (w.p("ring.prio"), CAP, w.p("ring.state"), w.p("ring.index_out"), w.t["ring.index_out"].numel() * 8, s),
     ("ring.index_out",)),
    ("gbl_replay_batch_prio", lambda w, s: (w.p("ring.obs"), w.p("ring.visits"), w.p("ring.meta"), CAP, w.p("ring.state"), w.p("ring.prio"),
                                            w.p("ring.index"), w.p("draw.priority"), w.p("draw.prio_total"), 0, B, nat.SYMMETRIES - 1, 9, 0, 2,
                                            *(w.p(k) for k in _DRAW_OUT), s), _DRAW_OUT + ("draw.priority", "draw.prio_total")),
    ("gbl_replay_importance", lambda w, s: (w.p("drawn.priority"), B, 0.5, w.p("out.weights"), s), ("out.weights",)),
    ("gbl_tb_prepare", lambda w, s: (w.c["inv"], w.p("tb.aux_out"), s), ("tb.aux_out",)),
    ("gbl_tb_sweep", lambda w, s: (*_table(w, "tb.part"), w.p("tb.sweep_out"), 0, w.c["positions"], w.c["sweep"], w.p("tb.decided"), s),
     ("tb.sweep_out", "tb.decided")),
    ("gbl_tb_index", lambda w, s: (w.c["inv"], w.p("tb.aux"), w.p("small.state"), w.p("small.to_move"), w.p("out.index64"), N, s), ("out.index64",)),
    ("gbl_tb_position", lambda w, s: (w.c["inv"], w.p("tb.aux"), w.p("small.index"), w.p("out.state"), N, s), ("out.state",)),
    ("gbl_tb_probe", lambda w, s: (*_table(w), w.p("small.state"), w.p("small.to_move"), None, w.p("out.outcome"), w.p("out.value8"),
                                   w.p("out.actions"), N, s), ("out.outcome", "out.value8", "out.actions")),
    ("gbl_tb_targets", lambda w, s: (*_table(w), *_rows(w), w.p("rows.visits"), w.p("rows.visits_out"), nat.ACTIONS, w.p("rows.z"), w.p("rows.z_out"), 1,
                                     nat.TB_TARGET_MODES["shortest"], 3, w.p("rows.tb_value"), None, w.p("rows.tally"), B, s),
     ("rows.visits_out", "rows.z_out", "rows.tb_value", "rows.tally")),
    ("gbl_reanalyse", lambda w, s: (_ev(w), ITER, 16, *_rows(w), w.p("rows.visits"), w.p("rows.visits_out"), nat.ACTIONS, w.p("rows.z"), 1,
                                    w.p("rows.root_value"), None, None, None, w.p("rows.drift"), w.p("rows.tally"), B, s),
     ("rows.visits_out", "rows.root_value", "rows.drift", "rows.tally")),
    ("gbl_reanalyse_gumbel", lambda w, s: (_ev(w), ITER, 16, 16, 1, 50, 23, 11, 0, 4, *_rows(w), w.p("rows.visits"), w.p("rows.visits_out"), nat.ACTIONS,
                                           w.p("rows.z"), 1, w.p("rows.root_value"), None, None, None, w.p("rows.drift"), w.p("rows.tally"),
                                           w.p("rows.gumbel"), B, s),
     ("rows.visits_out", "rows.root_value", "rows.drift", "rows.tally", "rows.gumbel")),
    ("gbl_symmetry_apply", lambda w, s: (w.p("sym"), 0, w.p("to_move"), w.p("state"), w.p("out.state"), w.p("obs"), w.p("out.obs"), w.p("mask"),
                                         w.p("out.mask"), w.p("rows.visits"), w.p("out.visits16"), None, None, w.p("actions"), w.p("out.actions_img"), N, s),
     ("out.state", "out.obs", "out.mask", "out.visits16", "out.actions_img")),
    ("gbl_training_batch", lambda w, s: (w.p("traj.observation"), w.p("traj.action_mask"), w.p("traj.visits"), w.p("traj.z"), w.p("traj.done"),
                                         w.p("traj.mover"), N, T, w.c["ply_stride"], w.c["tile_stride"], B, nat.SYMMETRIES - 1, 5, 0, 3,
                                         *(w.p(k) for k in _DRAW_OUT), s), _DRAW_OUT),
    ("gbl_outcome_targets", lambda w, s: (w.p("traj.done"), w.p("traj.rewards"), w.p("traj.mover"), w.p("traj.z_out"), w.p("traj.plies_left_out"),
                                          *_strides(w), T, s), ("traj.z_out", "traj.plies_left_out")),
    ("gbl_playout_values", lambda w, s: (w.p("state"), w.p("to_move"), None, 4, 16, 7, 0, 2, w.p("out.wins54"), w.p("out.losses54"), w.p("out.actions"),
                                         w.p("out.plies"), N, s), ("out.wins54", "out.losses54", "out.actions", "out.plies")),
    ("gbl_tree_search", lambda w, s: (w.p("state"), w.p("to_move"), None, ITER, 2, 16, 16, 7, 0, 2, w.p("out.visits54"), w.p("out.wins54"),
                                      w.p("out.losses54"), w.p("out.actions"), w.p("out.nodes"), w.p("out.plies"), N, s), _SEARCH_OUT + ("out.plies",)),
    ("gbl_evaluate", lambda w, s: (w.p("state"), w.p("to_move"), None, _ev(w), w.p("out.priors"), w.p("out.value"), w.p("out.logits"), N, s),
     ("out.priors", "out.value", "out.logits")),
    ("gbl_greedy", lambda w, s: (w.p("state"), w.p("to_move"), None, w.p("hist"), 2, w.p("out.actions"), w.p("out.cand"), w.p("out.fallback"), N, s),
     ("out.actions", "out.cand", "out.fallback")),
    ("gbl_sample", lambda w, s: (w.p("mask"), w.p("out.actions"), N, 7, 0, 3, s), ("out.actions",)),
    # ---- ... and the single-launch entry points that no capture test reached either ----
    ("gbl_reset", lambda w, s: (w.p("state"), w.p("to_move"), w.p("done"), w.p("out.winner"), N, s), _BOARDS + ("out.winner",)),
    ("gbl_legal_mask", lambda w, s: (w.p("state"), w.p("to_move"), w.p("out.mask"), N, s), ("out.mask",)),
    ("gbl_is_legal", lambda w, s: (w.p("state"), w.p("to_move"), w.p("actions"), w.p("out.legal"), N, s), ("out.legal",)),
    ("gbl_play_turn", lambda w, s: (w.p("state"), w.p("to_move"), w.p("actions"), N, s), ("state",)),
    ("gbl_winner", lambda w, s: (w.p("state"), w.p("out.winner"), N, s), ("out.winner",)),
    ("gbl_flatboard", lambda w, s: (w.p("state"), w.p("out.flat"), N, s), ("out.flat",)),
    ("gbl_covered", lambda w, s: (w.p("state"), w.p("out.covered"), N, s), ("out.covered",)),
    ("gbl_validate", lambda w, s: (w.p("state"), w.p("out.flags"), N, s), ("out.flags",)),
    ("gbl_observe", lambda w, s: (w.p("state"), w.p("to_move"), -1, w.p("out.obs"), N, s), ("out.obs",)),
    ("gbl_board_eval", lambda w, s: (w.p("state"), w.p("to_move"), w.p("actions"), w.p("out.record"), N, s), ("state", "out.record")),
    ("gbl_decode_obs", lambda w, s: (w.p("obs"), w.p("out.state"), w.p("out.to_move"), N, s), ("out.state", "out.to_move")),
    ("gbl_step", lambda w, s: (*_step_head(w), N, nat.ILLEGAL_NOOP, 1, s), _BOARDS + _PLY_OUT),
    ("gbl_step_into", lambda w, s: (*_step_head(w), w.p("out.actions"), w.p("out.done"), w.p("out.to_move"), N, nat.ILLEGAL_NOOP, 1, s),
     _BOARDS + _PLY_OUT + ("out.actions", "out.done", "out.to_move")),
    ("gbl_step_ex", lambda w, s: (*_step_head(w), w.p("out.actions"), w.p("out.done"), w.p("out.to_move"), w.p("out.status"), w.p("out.next"), 7, 0, 5,
                                  None, N, nat.ILLEGAL_NOOP, 1, s),
     _BOARDS + _PLY_OUT + ("out.actions", "out.done", "out.to_move", "out.status", "out.next")),
    ("gbl_sample_at", lambda w, s: (w.p("mask"), w.p("out.actions"), N, 7, 0, 3, None, s), ("out.actions",)),
    ("gbl_rollout", lambda w, s: (w.p("state"), w.p("to_move"), w.p("done"), w.p("out.actions"), w.p("out.winner"), w.p("out.reward"), w.p("out.mask"),
                                  w.p("out.obs"), N, 7, 0, 3, 3, nat.ILLEGAL_NOOP, w.p("counters"), w.p("turn"), s),
     _BOARDS + _PLY_OUT + ("counters", "out.actions")),
    ("gbl_greedy_act", lambda w, s: (w.p("state"), w.p("to_move"), None, w.p("hist"), 2, 7, 0, 3, w.p("out.actions"), w.p("out.chosen"), w.p("out.cand"),
                                     w.p("out.fallback"), N, s), ("hist", "out.actions", "out.chosen", "out.cand", "out.fallback")),
    ("gbl_greedy_act_at", lambda w, s: (w.p("state"), w.p("to_move"), None, w.p("hist"), 2, 7, 0, 3, None, w.p("out.actions"), w.p("out.chosen"),
                                        w.p("out.cand"), w.p("out.fallback"), N, s), ("hist", "out.actions", "out.chosen", "out.cand", "out.fallback")),
    ("gbl_collect", lambda w, s: (w.p("state"), w.p("to_move"), w.p("done"), *_win(w, *_WIN), *_strides(w), 7, 0, 3, None, T, nat.ILLEGAL_NOOP,
                                  w.p("counters"), w.p("turn"), s), _BOARDS + ("counters", "turn") + _WIN_OUT),
    ("gbl_collect_from", lambda w, s: (w.p("state"), w.p("to_move"), w.p("done"), w.p("actions"), *_win(w, *_WIN), *_strides(w), 7, 0, 3, None, T,
                                       nat.ILLEGAL_NOOP, w.p("counters"), w.p("turn"), s), _BOARDS + ("counters", "turn") + _WIN_OUT),
    ("gbl_collect_policy", lambda w, s: (w.p("state"), w.p("to_move"), w.p("done"), w.p("hist"), *_win(w, *_WIN, "chosen", "how", "candidates"),
                                         *_strides(w), 7, 0, 3, None, T, nat.POLICY_GREEDY2, nat.POLICY_RANDOM, 0, nat.ILLEGAL_NOOP, w.p("counters"),
                                         w.p("turn"), s),
     _BOARDS + ("hist", "counters", "turn", "win.chosen", "win.how", "win.candidates") + _WIN_OUT),
    ("gbl_tree_search_eval_noise", lambda w, s: (w.p("state"), w.p("to_move"), None, _ev(w), ITER, 16, 64, 7, 0, 2, *(w.p(k) for k in _SEARCH_OUT),
                                                 w.p("out.root_value"), w.p("out.priors"), w.p("out.mixed"), N, s),
     _SEARCH_OUT + ("out.root_value", "out.priors", "out.mixed")),
    ("gbl_tree_search_gumbel", lambda w, s: (w.p("state"), w.p("to_move"), None, _ev(w), ITER, 16, 16, 1, 50, 23, 7, 0, 2, *(w.p(k) for k in _SEARCH_OUT),
                                             w.p("out.root_value"), w.p("out.priors"), w.p("out.target"), w.p("out.gumbel"), N, s),
     _SEARCH_OUT + ("out.root_value", "out.priors", "out.target", "out.gumbel")),
]
NAMES = [name for name, _, _ in TABLE]

# the entry points a graph-capture test reached before this table: tests/test_gpu_parity.py (rollout, collect and the ply counter),
# tests/test_gpu_solver.py, tests/test_gpu_evaluator_edges.py, and the self-play family's own test_gpu_* files
ALREADY_CAPTURED = ("gbl_rollout_at", "gbl_counter_add", "gbl_collect_from_ex", "gbl_solve", "gbl_tree_search_eval", "gbl_collect_search",
                    "gbl_collect_search_eval", "gbl_collect_search_solve", "gbl_collect_search_noise", "gbl_collect_search_cap",
                    "gbl_collect_search_gumbel", "gbl_collect_search_tb", "gbl_collect_gumbel_solve", "gbl_collect_gumbel_tb")


def is_helper(name: str) -> bool:
    """The symbols include/gobblet_hip.h's "Conventions" block keeps out of "only enqueue on `stream`": the allocators, the placement
    probe, and the queries that launch nothing."""
    return name.startswith(("gbl_pinned_", "gbl_block_")) or name in ("gbl_placement_probe", "gbl_device_memory", "gbl_last_error", "gbl_layout_info") \
        or name.endswith(("_bytes", "_layout", "_variant"))


def run_eager(w: World, name: str, flavour_lib, stream) -> None:
    """The entry's one raw call; on the host flavour (``_HostFlavour``) a failure raises, on the device the code is checked here."""
    make = dict((n, m) for n, m, _ in TABLE)[name]
    rc = getattr(flavour_lib, name)(*make(w, stream))
    assert rc == nat.OK, (name, rc, nat.lib().gbl_last_error().decode())


def comparable(snap: dict) -> dict:
    """What the ABI defines of a snapshot: everything but the workspaces, whose bytes it leaves unspecified, and of the striped
    ``counters`` their totals (the device spreads its tallies over the stripes, the host flavour adds to the first one)."""
    return {k: (v.sum(0) if k == "counters" else v) for k, v in snap.items() if not k.startswith("ws.")}
