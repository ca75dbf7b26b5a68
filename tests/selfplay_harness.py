"""What the tests of the seven self-play entry points (gbl_collect_search, _eval, _solve, _noise, _cap, _gumbel, _tb; either flavour)
share: the output tables, the trajectory geometry, ONE argument list (by name, ordered by nat.SELFPLAY_ARGS), one runner on host arrays
and one on the device (every output filled with -7 / 99 first: nothing outside the cells may be written), the comparison, and the
evaluator helpers.  A plain module: no fixtures."""
import ctypes as C

import numpy as np

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from gobblet_rl_amd._selfplay import TRAJ_BUFFERS
from tests.search_harness import DEV, PAD
from tests.search_harness import same as same_arrays

SCALARS = (("actions", np.int32, ()), ("winner", np.int8, ()), ("rewards", np.int8, (2,)), ("done", np.int8, ()),
           ("to_move", np.int8, ()), ("action_mask", np.int8, (54,)), ("observation", np.int8, (117,)), ("visits", np.int16, (54,)),
           ("value", np.int32, ()), ("nodes", np.int32, ()), ("how", np.int8, ()), ("mover", np.int8, ()))
EVAL_NAMES = SCALARS + (("root_value", np.int32, ()), ("priors", np.uint8, (54,)))
SOLVE_NAMES = EVAL_NAMES + (("outcomes", np.int8, (54,)), ("proven", np.int8, ()))
JUDGE_NAMES = (("tb_outcomes", np.int8, (54,)), ("tb_value", np.int8, ()), ("tb_played", np.int8, ()))
# entry point -> its outputs (name = the key of BatchedGobblet.trajectory_buffers, dtype, a cell's shape)
NAMES = {"search": SCALARS, "eval": EVAL_NAMES, "solve": SOLVE_NAMES, "noise": SOLVE_NAMES, "cap": SOLVE_NAMES, "gumbel": EVAL_NAMES,
         "tb": SOLVE_NAMES + JUDGE_NAMES}
CODES = {"random": nat.POLICY_RANDOM, "tree": nat.POLICY_TREE, "eval": nat.POLICY_EVAL_TREE, "tb": nat.POLICY_TABLEBASE}


def symbol(entry):
    return "gbl_collect_search" + ("" if entry == "search" else "_" + entry)


def strides(n, T, layout):
    tiles = -(-n // 64)
    if layout == "time":
        slot = tiles * 64 + 64  # (a padded slot: the stride is not the board count)
        return slot, 64, T * slot
    return 64, 64 * T, tiles * T * 64


def cells(n, T, layout):
    ps, ts, _ = strides(n, T, layout)
    b = np.arange(n)
    return np.arange(T)[:, None] * ps + (b // 64) * ts + b % 64  # (T, n)


def geometry(n, T, layout, override=None):
    """(ply_stride, tile_stride, the cells an array must have, cell(t, b) as (T, n)) of the compact layout, or of
    override = (ply_stride, tile_stride), in cells."""
    ps, ts, total = strides(n, T, layout)
    if override is not None:
        ps, ts = override
        total = (T - 1) * ps + (-(-n // 64) - 1) * ts + 64
    b = np.arange(n)
    return ps, ts, total, np.arange(T)[:, None] * ps + (b // 64) * ts + b % 64


class Compact:
    """Where a runner keeps its trajectory outputs: an array each, filled with -7 / 99, `pad` rows of the same on either side.  A test
    with a geometry of its own brings another store of the same two methods (tests/test_gpu_far_offsets.py)."""

    def __init__(self, put, get, pad):
        self.put, self.get, self.pad, self.full = put, get, pad, {}

    def array(self, k, dt, tail, total):
        """The array of output k, from its cell 0."""
        self.full[k] = self.put(np.full((total + 2 * self.pad,) + tail, 99 if dt == np.uint8 else -7, dt))
        return self.full[k][self.pad:]

    def cells(self, at, total):
        """{k: (T, n, ...)} on the host, after checking that nothing outside the cells is written, the canaries on either side included."""
        untouched = np.ones(total + 2 * self.pad, bool)
        untouched[at.ravel() + self.pad] = False
        host = {k: self.get(v) for k, v in self.full.items()}
        for k, v in host.items():
            assert (v[untouched] == (99 if v.dtype == np.uint8 else -7)).all(), "output %s was written outside its cells" % k
        return {k: v[self.pad:][at] for k, v in host.items()}


def call_args(entry, ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, X, sample_plies, illegal_mode, counters, tn, stream,
              its=(0, 0), pls=(0, 0), M=0, evs=(None, None), deps=(0, 0), noise=(0, 0), fast=(0, 0), share=(256, 256), considered=(0, 0),
              gumbel_noise=0, visit_offset=0, scale=0, tb=None, mode=0, count=1):
    """The argument list of gbl(_cpu)_collect_search ("search") or of its _`entry`: every value a member of the family may take, by
    the ABI's name, of which nat.SELFPLAY_ARGS picks and orders the entry point's own.  ptr(x) turns an array (or None) into a pointer,
    evs are gbl_evaluator structs (or None), tb a tests.selfplay_tb_harness.Table (or None: NULL for all three)."""
    name = symbol(entry)
    ev0, ev1 = (None if e is None else C.addressof(e) for e in evs)
    every = dict(
        state=ptr(st), to_move=ptr(tm), done=ptr(dn), **{arg: ptr(traj.get(k)) for arg, k in TRAJ_BUFFERS.items()}, n=n, ply_stride=ps,
        tile_stride=ts, seed=seed, env_base=env_base, ply0=ply0, ply_dev=ptr(pd), plies=T, policy0=CODES[pols[0]], policy1=CODES[pols[1]],
        ev0=ev0, ev1=ev1, iterations0=its[0], iterations1=its[1], playouts0=pls[0], playouts1=pls[1], max_plies=M, solve_depth0=deps[0],
        solve_depth1=deps[1], noise0=int(noise[0]), noise1=int(noise[1]), explore=X, sample_plies=sample_plies, illegal_mode=illegal_mode,
        counters=ptr(counters), turn=ptr(tn), fast_iterations0=int(fast[0]), fast_iterations1=int(fast[1]), full_share0=int(share[0]),
        full_share1=int(share[1]), considered0=int(considered[0]), considered1=int(considered[1]), gumbel_noise=int(gumbel_noise),
        visit_offset=int(visit_offset), scale=int(scale), inventory=None if tb is None else tb.inv, aux=None if tb is None else ptr(tb.aux),
        table=None if tb is None else ptr(tb.table), tb_mode=mode, tb_count=count, stream=stream)
    return nat.selfplay_args(name, **{k: every[k] for k, _ in nat.SELFPLAY_ARGS[name]})


def _run(entry, f, ok, put, get, ptr, pad, stream, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0,
         ply_dev, keep, counters, nets, strides=None, store=None, **sides):
    """strides: (ply_stride, tile_stride) in place of the compact ones of `layout`; store: where the outputs live (a Compact of this
    runner's put / get / pad unless the caller brings one)."""
    n = len(st)
    ps, ts, total, at = geometry(n, T, layout, strides)
    store = Compact(put, get, pad) if store is None else store
    keep = [k for k, _, _ in NAMES[entry]] if keep is None else keep
    traj = {k: store.array(k, dt, tail, total) for k, dt, tail in NAMES[entry] if k in keep}
    st, tm, dn = put(np.ascontiguousarray(st, np.int8)), put(np.ascontiguousarray(tm, np.int8)), put(np.full(n, 5, np.int8))
    tn = None if turn is None else put(np.ascontiguousarray(turn, np.int32))
    pd = None if ply_dev is None else put(np.array([ply_dev], np.int32))
    evs = [None if net is None else net.struct() for net in nets]  # (alive until the call has returned)
    ok(f(*call_args(entry, ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, X, sample_plies, illegal_mode, counters, tn,
                    stream, evs=evs, **sides)))
    return store.cells(at, total), get(st), get(tm), get(dn), None if tn is None else get(tn)


def host_collect(entry, f, err, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev=None, keep=None,
                 counters=None, nets=(None, None), **sides):
    """`f` = gbl_cpu_collect_search* of `entry` on host arrays; only the outputs named in `keep` are given (None: all); sides: what
    call_args takes by keyword (its=, pls=, M=, deps=, noise=, fast=, share=, considered=, ..., tb=, mode=, count=) and _run's
    strides= / store=; nets: restatement Nets.  Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    def ok(rc):
        assert rc == 0, err()

    def ptr(a):
        return None if a is None else a.ctypes.data
    return _run(entry, f, ok, np.array, lambda a: a, ptr, 0, None, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base,
                ply0, ply_dev, keep, counters, nets, **sides)


def device_collect(entry, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev=None, keep=None,
                   counters=None, nets=(None, None), **sides):
    """gbl_collect_search* of `entry` on the device, every output between canaries; nets: DeviceNets; counters: a device tensor; the
    same return value as host_collect."""
    import torch
    name = symbol(entry)

    def get(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return _run(entry, getattr(nat.lib(), name), lambda rc: nat.check(rc, name), lambda a: torch.from_numpy(a).to(DEV), get, nat.ptr, PAD,
                nat.current_stream(DEV), st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev, keep, counters,
                nets, **sides)


def same(got, exp):
    same_arrays(got[0], exp[0])
    for name, g, e in zip(("state", "to_move", "done", "turn"), got[1:], exp[1:]):
        if g is not None:
            assert np.array_equal(g, e), name


class DeviceNet:
    """A restatement Net with its four arrays on the device."""

    def __init__(self, net):
        import torch
        self.net = net
        self.arrays = [torch.from_numpy(a).to(DEV) for a in (net.w1, net.b1, net.w2, net.b2)]
        assert all(a.data_ptr() % 16 == 0 for a in self.arrays)

    def struct(self):
        return self.net.struct(self.arrays)


def _evaluator(net, device="cpu"):
    return G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, net.shift1, net.shift_p, net.shift_v, device=device)
