"""What the tests of gbl_tree_search_gumbel and gbl_collect_search_gumbel (either flavour) share, on top of tests/search_harness.py and
tests/selfplay_harness.py: the single-decision entry point's line in the harness's table (so that `run` serves it, canaries and all),
the self-play argument list (that of gbl_collect_search_eval, then the rule's five), one runner on host arrays and one on the device
(every output filled with -7 / 99 first and, on the device, kept between canaries), and the boards.  A plain module: no fixtures."""
import ctypes as C

import numpy as np

import oracle
from gobblet_rl_amd import _native as nat
from tests import search_harness as SH
from tests.search_harness import DEV, PAD
from tests.selfplay_harness import CODES, EVAL_NAMES, cells, strides

SH.ENTRIES.setdefault("tree_search_gumbel", (
    ("iterations", "explore", "considered", "gumbel_noise", "visit_offset", "scale", "seed", "env_base", "call"), True,
    SH._EVAL_TREE + (SH._out("target", np.uint8, (54,)), SH._out("gumbel", np.int16, (54,)))))
GUMBEL_NAMES = tuple(o[0] for o in SH.ENTRIES["tree_search_gumbel"][2])

PAIRS = ((1, 8), (2, 8), (3, 8), (4, 16), (5, 12), (16, 16), (16, 64), (54, 16))  # (considered, iterations)


def rule_boards(midgames):
    """The roots of the rule's tests from (state, to_move) midgames: two empty boards (54 candidates, either mover), the midgames, and
    eight more rows under masks that keep 27, 2, 1 and 0 candidates of an empty board and of a midgame.  Returns (state, to_move,
    mask, {candidates: a board that has so many})."""
    ms, mt = midgames
    st = np.concatenate([np.zeros((2, 27), np.int8), ms, np.zeros((4, 27), np.int8), ms[:4]])
    tm = np.concatenate([np.array([0, 1], np.int8), mt, np.array([0, 1, 0, 1], np.int8), mt[:4]])
    mask = np.ones((len(st), 54), np.int8)
    first, where = 2 + len(ms), {54: 0}
    for i, keep in enumerate((27, 2, 1, 0, 27, 2, 1, 0)):
        b = first + i
        legal = np.flatnonzero(oracle.legal_mask(st[b], int(tm[b])))
        assert len(legal) >= keep
        mask[b] = 0
        mask[b, legal[::-1][:keep]] = 1  # (the highest actions: the lowest-action tie-break has something to do)
        where.setdefault(keep, b)
    return np.ascontiguousarray(st), np.ascontiguousarray(tm), mask, where


def call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, evs, its, X, sample_plies, illegal_mode, counters, tn,
              considered, noise, visit_offset, scale, stream):
    """The argument list of gbl(_cpu)_collect_search_gumbel."""
    return [ptr(st), ptr(tm), ptr(dn), *[ptr(traj.get(k)) for k, _, _ in EVAL_NAMES], n, ps, ts, seed, env_base, ply0, ptr(pd), T,
            CODES[pols[0]], CODES[pols[1]], *[None if e is None else C.addressof(e) for e in evs], its[0], its[1], X, sample_plies,
            illegal_mode, ptr(counters), ptr(tn), int(considered[0]), int(considered[1]), int(noise), int(visit_offset), int(scale), stream]


def _run(f, ok, put, get, ptr, pad, stream, st, tm, turn, T, pols, nets, its, considered, noise, visit_offset, scale, X, sample_plies,
         illegal_mode, layout, seed, env_base, ply0, ply_dev, keep, counters):
    n = len(st)
    ps, ts, total = strides(n, T, layout)
    keep = [k for k, _, _ in EVAL_NAMES] if keep is None else keep
    full = {k: put(np.full((total + 2 * pad,) + tail, 99 if dt == np.uint8 else -7, dt)) for k, dt, tail in EVAL_NAMES if k in keep}
    traj = {k: v[pad:] for k, v in full.items()}
    st, tm, dn = put(np.ascontiguousarray(st, np.int8)), put(np.ascontiguousarray(tm, np.int8)), put(np.full(n, 5, np.int8))
    tn = None if turn is None else put(np.ascontiguousarray(turn, np.int32))
    pd = None if ply_dev is None else put(np.array([ply_dev], np.int32))
    evs = [None if net is None else net.struct() for net in nets]  # (alive until the call has returned)
    ok(f(*call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, evs, its, X, sample_plies, illegal_mode, counters, tn,
                    considered, noise, visit_offset, scale, stream)))
    at = cells(n, T, layout)
    untouched = np.ones(total + 2 * pad, bool)
    untouched[at.ravel() + pad] = False
    host = {k: get(v) for k, v in full.items()}
    for k, v in host.items():  # (nothing outside the cells is written, the canaries on either side included)
        assert (v[untouched] == (99 if v.dtype == np.uint8 else -7)).all(), "output %s was written outside its cells" % k
    return {k: v[pad:][at] for k, v in host.items()}, get(st), get(tm), get(dn), None if tn is None else get(tn)


def host_collect_gumbel(st, tm, turn, T, pols, nets, its, considered, noise=1, visit_offset=50, scale=23, X=16, sample_plies=0,
                        illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, keep=None, counters=None):
    """gbl_cpu_collect_search_gumbel on host arrays; nets: restatement Nets; only the outputs named in `keep` are given (None: all).
    Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    L = nat.cpu_raw()

    def ok(rc):
        assert rc == 0, L.gbl_cpu_last_error()

    def ptr(a):
        return None if a is None else a.ctypes.data
    return _run(L.gbl_cpu_collect_search_gumbel, ok, np.array, lambda a: a, ptr, 0, None, st, tm, turn, T, pols, nets, its, considered, noise,
                visit_offset, scale, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev, keep, counters)


def device_collect_gumbel(st, tm, turn, T, pols, nets, its, considered, noise=1, visit_offset=50, scale=23, X=16, sample_plies=0,
                          illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, keep=None, counters=None):
    """gbl_collect_search_gumbel on the device, every output between canaries; nets: DeviceNets."""
    import torch

    def get(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return _run(nat.lib().gbl_collect_search_gumbel, lambda rc: nat.check(rc, "gbl_collect_search_gumbel"),
                lambda a: torch.from_numpy(a).to(DEV), get, nat.ptr, PAD, nat.current_stream(DEV), st, tm, turn, T, pols, nets, its,
                considered, noise, visit_offset, scale, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev, keep, counters)
