"""What the tests of gbl_collect_search_cap (either flavour) share, on top of tests/selfplay_harness.py (whose one runner serves the
entry point as "cap"): the full share, and the runner calls under the cap's own argument order and defaults.  A plain module: no fixtures."""
from gobblet_rl_amd import _native as nat
from tests.selfplay_harness import device_collect, host_collect

FULL = 256  # the share at which every ply is full


def host_collect_cap(st, tm, turn, T, pols, nets, its, fast, share, deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                     illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, **kw):
    """gbl_cpu_collect_search_cap on host arrays; nets: restatement Nets; kw: ply_dev=, keep=, counters=, strides=, store=.
    Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    L = nat.cpu_raw()
    return host_collect("cap", L.gbl_cpu_collect_search_cap, L.gbl_cpu_last_error, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout,
                        seed, env_base, ply0, nets=nets, its=its, deps=deps, noise=noise, fast=fast, share=share, **kw)


def device_collect_cap(st, tm, turn, T, pols, nets, its, fast, share, deps=(0, 0), noise=(0, 0), X=16, sample_plies=0,
                       illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, **kw):
    """gbl_collect_search_cap on the device, every output between canaries; nets: DeviceNets."""
    return device_collect("cap", st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, nets=nets, its=its,
                          deps=deps, noise=noise, fast=fast, share=share, **kw)
