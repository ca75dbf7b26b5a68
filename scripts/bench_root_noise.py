#!/usr/bin/env python3
"""Root noise (gbl_tree_search_eval_noise / gbl_collect_search_noise): what carrying the weight through k_collect_solve costs, what
the noise itself costs, and how many different games it buys.  Shapes as scripts/bench_selfplay_solve.py: the stationary
masked-random mix (BatchedGobblet(N, seed=11).rollout(64), BASELINE config 5), evaluator against evaluator with one seeded integer
network (H 64), 64 iterations, explore 16, sample_plies 0, T = 16; both sides guarded at depth D (0: no guard).

    python scripts/bench_root_noise.py [out.json] [--parent lib.so]   on the GPU (default out: profiles/r18/root_noise.json)
    python scripts/bench_root_noise.py --host [out.json]              the distinct-games census on the host flavour (no GPU)

  (p) parent   gbl_collect_search_solve of a library built from the PARENT commit (--parent: its libgobblet_hip.so; without it the
               comparison is recorded as not measured);
  (s) solve    gbl_collect_search_solve of this build: (s) against (p) is the price of carrying the weight;
  (z) zero     gbl_collect_search_noise with weights (0, 0): the same kernel through the new entry point;
  (n) noise    gbl_collect_search_noise with weights (64, 64): (n) against (z) is the price of the noise itself.
Method: HIP events, one warm-up each, then 5 repetitions alternating (p), (s), (z), (n) in one process; median, min and max; the
state is restored outside the timed region.  (s) may be slower than (p) by no more than (p)'s own min-max spread.  Before anything
is timed, (p), (s) and (z) are compared array by array.

--host: 4 096 boards from the empty position, the same seeded network, 16 plies, sample_plies 0 and 4, weights 0 / 64 / 128 on both
sides: the number of distinct action sequences, and the share of plies whose action differs from the noise-free window's."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
from bench_selfplay_eval import seeded_evaluator  # noqa: E402
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402
from bench_selfplay_solve import PLY0, Runner, H, I, X  # noqa: E402
from bench_solver import merge  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r18", "root_noise.json")
POINTS = tuple((n, d) for n in (4096, 65536) for d in (0, 3))  # (boards, depth)
ARRAYS = ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation", "visits", "value", "nodes", "how", "mover",
          "root_value", "priors", "outcomes", "proven")


class NoiseRunner(Runner):
    """Runner's position and arrays; the guarded launch of this build, of a parent build, and the noised one."""

    def __init__(self, *args, parent=None, **kw):
        super().__init__(*args, **kw)
        self.parent_lib = parent

    def _solve(self, fn, a, name):
        e = C.addressof(self.struct)
        nat.check(fn(*self._head(a), nat.ptr(a["outcomes"]), nat.ptr(a["proven"]), self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T,
                     nat.POLICY_EVAL_TREE, nat.POLICY_EVAL_TREE, e, e, self.I, self.I, self.depth, self.depth, X, 0, nat.ILLEGAL_NOOP, None,
                     None, self.stream), name)

    def _noise(self, a, w):
        e = C.addressof(self.struct)
        nat.check(nat.lib().gbl_collect_search_noise(
            *self._head(a), nat.ptr(a["outcomes"]), nat.ptr(a["proven"]), self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T,
            nat.POLICY_EVAL_TREE, nat.POLICY_EVAL_TREE, e, e, self.I, self.I, self.depth, self.depth, w, w, X, 0, nat.ILLEGAL_NOOP, None, None,
            self.stream), "gbl_collect_search_noise")

    def solve(self):
        self._solve(nat.lib().gbl_collect_search_solve, self.a, "gbl_collect_search_solve")

    def parent(self):
        self._solve(self.parent_lib.gbl_collect_search_solve, self.b, "gbl_collect_search_solve (parent)")

    def zero(self):
        self._noise(self.c, 0)

    def noise(self):
        self._noise(self.c, 64)

    def check_same(self):
        """(p), (s) and (z) write the same arrays; (n) plays other games."""
        n = self.n
        self.restore(); self.solve(); torch.cuda.synchronize()
        end = (self.st.clone(), self.tm.clone())
        self.restore(); self.zero(); torch.cuda.synchronize()
        for k in ARRAYS:
            assert torch.equal(self.a[k][:, :n], self.c[k][:, :n]), k
        assert torch.equal(end[0], self.st) and torch.equal(end[1], self.tm)
        if self.parent_lib is not None:
            self.restore(); self.parent(); torch.cuda.synchronize()
            for k in ARRAYS:
                assert torch.equal(self.a[k][:, :n], self.b[k][:, :n]), k
        self.restore(); self.noise(); torch.cuda.synchronize()
        return float((self.a["actions"][:, :n] != self.c["actions"][:, :n]).float().mean())


def load_parent(path):
    L = C.CDLL(os.path.abspath(path))
    for name in ("gbl_collect_search_solve", "gbl_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L


def device(path, parent_path):
    parent = load_parent(parent_path) if parent_path else None
    names = (("parent",) if parent is not None else ()) + ("solve", "zero", "noise")
    rows, cache = [], {}
    for n, d in POINTS:
        if n not in cache:
            cache = {n: states(n)}
        r = NoiseRunner(*cache[n], I, seeded_evaluator(H), d, parent=parent)
        moved = r.check_same()
        t = r.time(reps=REPS, names=names)
        row = {"boards": n, "depth": d, "iterations": I, "hidden": H, "plies": T, "explore": X,
               "solve_ms": stats(t["solve"]), "zero_ms": stats(t["zero"]), "noise_ms": stats(t["noise"]),
               "noise_over_zero": stats(t["noise"])["median"] / stats(t["zero"])["median"],
               "noise_within_zero_spread": within_spread(t["noise"], t["zero"]),
               "actions_changed_by_noise": moved}
        if parent is not None:
            p = stats(t["parent"])
            row.update(parent_ms=p, parent_spread_ms=p["max"] - p["min"], solve_over_parent=stats(t["solve"])["median"] / p["median"],
                       solve_within_parent_spread=within_spread(t["solve"], t["parent"]))
        else:
            row.update(parent_ms="NOT MEASURED")
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r
        torch.cuda.empty_cache()
        merge(path, "rows", rows)
    merge(path, "device", torch.cuda.get_device_name(0))
    merge(path, "method", "HIP events; evaluator against evaluator (seeded int8 weights, H %d, %d iterations) from the same C5 position, state "
          "restored outside the timed region; one warm-up each, then %d repetitions alternating parent / solve / zero / noise in one "
          "process; ms per %d plies; parent = gbl_collect_search_solve of a library built from the parent commit" % (H, I, REPS, T))
    print("wrote", path)


def host(path, boards=4096, plies=16):
    nat.cpu_raw().gbl_cpu_set_threads(16)
    ev = seeded_evaluator(H, "cpu")
    rows = []
    for sample_plies in (0, 4):
        base = None
        for share in (0.0, 0.25, 0.5):
            t0 = time.perf_counter()
            env = G.BatchedGobblet(boards, "cpu", auto_reset=True, seed=11, track_turn=True)
            tr = env.collect(plies, policies=("evaluator", "evaluator"), out="fresh",
                             search=dict(evaluator=ev, iterations=I, explore=X, sample_plies=sample_plies, noise=share))
            acts = tr["actions"].numpy().T
            if base is None:
                base = acts
            rows.append({"boards": boards, "plies": plies, "iterations": I, "sample_plies": sample_plies, "weight": round(256 * share),
                         "distinct_action_sequences": len({r.tobytes() for r in acts}),
                         "plies_differing_from_noise_free": float((acts != base).mean()), "seconds": time.perf_counter() - t0})
            print(rows[-1], flush=True)
    merge(path, "distinct_games_host_flavour", {"network": "seeded int8 weights, H %d (untrained)" % H, "start": "the empty position",
                                                "rows": rows})
    print("wrote", path)


def main():
    args = sys.argv[1:]
    is_host = "--host" in args
    args = [a for a in args if a != "--host"]
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = args[i + 1]
        del args[i:i + 2]
    path = args[0] if args else DEFAULT_OUT
    host(path) if is_host else device(path, parent)


if __name__ == "__main__":
    main()
