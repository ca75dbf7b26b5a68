"""What the tests of gbl_collect_search_tb (either flavour) share, on top of tests/selfplay_harness.py (whose one runner serves the
entry point as "tb"): the output table with the three judge arrays, the table as the entry point takes it, the runner calls under the
entry point's own argument order and defaults, the start boards and the table sources.  A plain module: no fixtures."""
import numpy as np

from gobblet_rl_amd import _native as nat
from tests import tablebase_harness as TH
from tests import tb_targets_harness as TT
from tests.selfplay_harness import CODES, JUDGE_NAMES, NAMES, SOLVE_NAMES, device_collect, host_collect  # noqa: F401  (re-exported)

TB_NAMES = NAMES["tb"]  # SOLVE_NAMES + JUDGE_NAMES
MODES = {"result": 0, "shortest": 1}


class Table:
    """A table as the entry point takes it: inv (int32[3] on the host), aux and table (arrays where the flavour runs)."""

    def __init__(self, inventory, aux, table):
        self.inventory, self.inv, self.aux, self.table = tuple(inventory), TH.inv_array(inventory), aux, table


def host_collect_tb(tb, st, tm, turn, T, pols, nets=(None, None), its=(0, 0), deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                    illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, mode=0, count=1, keep=None, **kw):
    """gbl_cpu_collect_search_tb on host arrays; tb: a Table of host arrays (or None); nets: restatement Nets; only the outputs named
    in `keep` are given (None: all); kw: counters=, strides=, store=.  Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    L = nat.cpu_raw()
    return host_collect("tb", L.gbl_cpu_collect_search_tb, L.gbl_cpu_last_error, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout,
                        seed, env_base, ply0, ply_dev, keep, nets=nets, its=its, deps=deps, noise=noise, tb=tb, mode=mode, count=count, **kw)


def device_collect_tb(tb, st, tm, turn, T, pols, nets=(None, None), its=(0, 0), deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                      illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, mode=0, count=1, keep=None, **kw):
    """gbl_collect_search_tb on the device, every output between canaries; tb: a Table of device tensors; nets: DeviceNets."""
    return device_collect("tb", st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev, keep, nets=nets,
                          its=its, deps=deps, noise=noise, tb=tb, mode=mode, count=count, **kw)


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
