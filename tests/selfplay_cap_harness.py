"""What the tests of gbl_collect_search_cap (either flavour) share, on top of tests/selfplay_harness.py: the argument list (that of
gbl_collect_search_noise, then the cap's four), one runner on host arrays and one on the device (every output filled with -7 / 99
first and, on the device, kept between canaries: nothing outside the cells may be written).  A plain module: no fixtures."""
import ctypes as C

import numpy as np

from gobblet_rl_amd import _native as nat
from tests.search_harness import DEV, PAD
from tests.selfplay_harness import CODES, SOLVE_NAMES, Compact, geometry

FULL = 256  # the share at which every ply is full


def call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, evs, its, deps, noise, X, sample_plies, illegal_mode,
              counters, tn, fast, share, stream):
    """The argument list of gbl(_cpu)_collect_search_cap."""
    return [ptr(st), ptr(tm), ptr(dn), *[ptr(traj.get(k)) for k, _, _ in SOLVE_NAMES], n, ps, ts, seed, env_base, ply0, ptr(pd), T,
            CODES[pols[0]], CODES[pols[1]], *[None if e is None else C.addressof(e) for e in evs], its[0], its[1], deps[0], deps[1],
            int(noise[0]), int(noise[1]), X, sample_plies, illegal_mode, ptr(counters), ptr(tn), int(fast[0]), int(fast[1]), int(share[0]),
            int(share[1]), stream]


def _run(f, ok, put, get, ptr, pad, stream, st, tm, turn, T, pols, nets, its, deps, noise, fast, share, X, sample_plies, illegal_mode, layout,
         seed, env_base, ply0, ply_dev, keep, counters, strides=None, store=None):
    n = len(st)
    ps, ts, total, at = geometry(n, T, layout, strides)
    store = Compact(put, get, pad) if store is None else store
    keep = [k for k, _, _ in SOLVE_NAMES] if keep is None else keep
    traj = {k: store.array(k, dt, tail, total) for k, dt, tail in SOLVE_NAMES if k in keep}
    st, tm, dn = put(np.ascontiguousarray(st, np.int8)), put(np.ascontiguousarray(tm, np.int8)), put(np.full(n, 5, np.int8))
    tn = None if turn is None else put(np.ascontiguousarray(turn, np.int32))
    pd = None if ply_dev is None else put(np.array([ply_dev], np.int32))
    evs = [None if net is None else net.struct() for net in nets]  # (alive until the call has returned)
    ok(f(*call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, evs, its, deps, noise, X, sample_plies, illegal_mode,
                    counters, tn, fast, share, stream)))
    return store.cells(at, total), get(st), get(tm), get(dn), None if tn is None else get(tn)


def host_collect_cap(st, tm, turn, T, pols, nets, its, fast, share, deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                     illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, keep=None, counters=None, strides=None, store=None):
    """gbl_cpu_collect_search_cap on host arrays; nets: restatement Nets; only the outputs named in `keep` are given (None: all).
    Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    L = nat.cpu_raw()

    def ok(rc):
        assert rc == 0, L.gbl_cpu_last_error()

    def ptr(a):
        return None if a is None else a.ctypes.data
    return _run(L.gbl_cpu_collect_search_cap, ok, np.array, lambda a: a, ptr, 0, None, st, tm, turn, T, pols, nets, its, deps, noise, fast,
                share, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev, keep, counters, strides, store)


def device_collect_cap(st, tm, turn, T, pols, nets, its, fast, share, deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                       illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, ply_dev=None, keep=None, counters=None, strides=None, store=None):
    """gbl_collect_search_cap on the device, every output between canaries; nets: DeviceNets."""
    import torch

    def get(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return _run(nat.lib().gbl_collect_search_cap, lambda rc: nat.check(rc, "gbl_collect_search_cap"), lambda a: torch.from_numpy(a).to(DEV),
                get, nat.ptr, PAD, nat.current_stream(DEV), st, tm, turn, T, pols, nets, its, deps, noise, fast, share, X, sample_plies,
                illegal_mode, layout, seed, env_base, ply0, ply_dev, keep, counters, strides, store)
