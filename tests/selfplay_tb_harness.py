"""What the tests of gbl_collect_search_tb (either flavour) share, on top of tests/selfplay_harness.py: the output table with the three
judge arrays, the argument list, one runner on host arrays and one on the device (every output filled with -7 / 99 first and, on the
device, kept between canaries), the start boards and the table sources.  A plain module: no fixtures."""
import ctypes as C

import numpy as np

from gobblet_rl_amd import _native as nat
from tests import tablebase_harness as TH
from tests import tb_targets_harness as TT
from tests.search_harness import DEV, PAD
from tests.selfplay_harness import SOLVE_NAMES, Compact, geometry

JUDGE_NAMES = (("tb_outcomes", np.int8, (54,)), ("tb_value", np.int8, ()), ("tb_played", np.int8, ()))
TB_NAMES = SOLVE_NAMES + JUDGE_NAMES
CODES = {"random": nat.POLICY_RANDOM, "eval": nat.POLICY_EVAL_TREE, "tb": nat.POLICY_TABLEBASE}
MODES = {"result": 0, "shortest": 1}


class Table:
    """A table as the entry point takes it: inv (int32[3] on the host), aux and table (arrays where the flavour runs)."""

    def __init__(self, inventory, aux, table):
        self.inventory, self.inv, self.aux, self.table = tuple(inventory), TH.inv_array(inventory), aux, table


def call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, evs, its, deps, noise, X, sample_plies, illegal_mode,
              counters, tn, tb, mode, count, stream):
    """The argument list of gbl(_cpu)_collect_search_tb; tb: a Table or None (NULL for all three)."""
    return [ptr(st), ptr(tm), ptr(dn), *[ptr(traj.get(k)) for k, _, _ in SOLVE_NAMES], n, ps, ts, seed, env_base, ply0, ptr(pd), T,
            CODES[pols[0]], CODES[pols[1]], *[None if e is None else C.addressof(e) for e in evs], its[0], its[1], deps[0], deps[1],
            int(noise[0]), int(noise[1]), X, sample_plies, illegal_mode, ptr(counters), ptr(tn),
            None if tb is None else tb.inv, None if tb is None else ptr(tb.aux), None if tb is None else ptr(tb.table), mode, count,
            *[ptr(traj.get(k)) for k, _, _ in JUDGE_NAMES], stream]


def _run(f, ok, put, get, ptr, pad, stream, tb, st, tm, turn, T, pols, nets, its, deps, noise, X, sample_plies, illegal_mode, layout, seed,
         env_base, ply0, ply_dev, mode, count, keep, counters, strides=None, store=None):
    n = len(st)
    ps, ts, total, at = geometry(n, T, layout, strides)
    store = Compact(put, get, pad) if store is None else store
    keep = [k for k, _, _ in TB_NAMES] if keep is None else keep
    traj = {k: store.array(k, dt, tail, total) for k, dt, tail in TB_NAMES if k in keep}
    st, tm, dn = put(np.ascontiguousarray(st, np.int8)), put(np.ascontiguousarray(tm, np.int8)), put(np.full(n, 5, np.int8))
    tn = None if turn is None else put(np.ascontiguousarray(turn, np.int32))
    pd = None if ply_dev is None else put(np.array([ply_dev], np.int32))
    evs = [None if net is None else net.struct() for net in nets]  # (alive until the call has returned)
    ok(f(*call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, evs, its, deps, noise, X, sample_plies, illegal_mode,
                    counters, tn, tb, mode, count, stream)))
    return store.cells(at, total), get(st), get(tm), get(dn), None if tn is None else get(tn)


def host_collect_tb(tb, st, tm, turn, T, pols, nets=(None, None), its=(0, 0), deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                    illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, mode=0, count=1, keep=None,
                    counters=None, strides=None, store=None):
    """gbl_cpu_collect_search_tb on host arrays; nets: restatement Nets; only the outputs named in `keep` are given (None: all).
    Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    L = nat.cpu_raw()

    def ok(rc):
        assert rc == 0, L.gbl_cpu_last_error()

    def ptr(a):
        return None if a is None else a.ctypes.data
    return _run(L.gbl_cpu_collect_search_tb, ok, np.array, lambda a: a, ptr, 0, None, tb, st, tm, turn, T, pols, nets, its, deps, noise, X,
                sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev, mode, count, keep, counters, strides, store)


def device_collect_tb(tb, st, tm, turn, T, pols, nets=(None, None), its=(0, 0), deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                      illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, mode=0, count=1, keep=None,
                      counters=None, strides=None, store=None):
    """gbl_collect_search_tb on the device, every output between canaries; tb: a Table of device tensors; nets: DeviceNets."""
    import torch

    def get(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return _run(nat.lib().gbl_collect_search_tb, lambda rc: nat.check(rc, "gbl_collect_search_tb"), lambda a: torch.from_numpy(a).to(DEV), get,
                nat.ptr, PAD, nat.current_stream(DEV), tb, st, tm, turn, T, pols, nets, its, deps, noise, X, sample_plies, illegal_mode, layout,
                seed, env_base, ply0, ply_dev, mode, count, keep, counters, strides, store)


def start_boards(host, n_positions, n_random, n_fresh, seed):
    """The three kinds of start boards in one batch: sampled quiet positions of the host's inventory seen by either mover, masked-random
    full-inventory boards (outside a small inventory: the a* == -1 path) and fresh boards.  (state, to_move, turn)."""
    p_st, p_tm = TH.sample_boards(host, n_positions, seed)
    _, r_st, r_tm = TT.random_play_rows(n_random, (3, 5, 6, 9), seed + 1)
    st = np.concatenate([p_st, r_st, np.zeros((n_fresh, 27), np.int8)]).astype(np.int8)
    tm = np.concatenate([p_tm, r_tm, np.zeros(n_fresh, np.int8)]).astype(np.int8)
    turn = (np.arange(len(st)) % 4).astype(np.int32)
    turn[len(st) - n_fresh:] = 0
    return np.ascontiguousarray(st), np.ascontiguousarray(tm), turn
