#!/usr/bin/env python3
"""Playout-cap randomisation (gbl_collect_search_cap): what a capped self-play window costs against the uncapped one, and what the
CAP = false instantiations cost against the parent commit's kernels.  Shapes as scripts/bench_root_noise.py: the stationary
masked-random mix (BatchedGobblet(N, seed=11).rollout(64), BASELINE config 5), evaluator against evaluator with one seeded integer
network (H 64), 64 iterations, explore 16, sample_plies 0, T = 16, noise weight 64 on both sides; both sides guarded at depth D (0: no
guard).

    python scripts/bench_selfplay_cap.py [out.json] [--parent lib.so]   on the GPU (default out: profiles/r28/selfplay_cap.json)

  (p) parent   gbl_collect_search_noise of a library built from the PARENT commit (--parent: scripts/build_variant.sh makes it from a
               checkout of that commit; without it the comparison is recorded as NOT MEASURED) -- the uncapped window every ratio is
               taken against;
  (n) noise    gbl_collect_search_noise of this build: the same instantiation, so (n) must lie inside (p)'s own min-max spread;
  (c16) (c8)   gbl_collect_search_cap with (fast_iterations, full_share) = (16, 64) and (8, 64) on both sides.
Method: HIP events, one warm-up each, then 5 repetitions alternating (p), (n), (c16), (c8) in one process; median, min and max; the
state is restored outside the timed region.  Before anything is timed, (p), (n) and the new entry point at shares (256, 256) are
compared array by array.  Kept rows: the cells of the window whose visits row is not zero (what gbl_training_batch and
gbl_replay_append can keep); evaluations: the sum of `nodes`."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gobblet_rl_amd import _native as nat  # noqa: E402
from bench_selfplay_eval import seeded_evaluator  # noqa: E402
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402
from bench_selfplay_solve import PLY0, Runner, H, I, X  # noqa: E402
from bench_solver import merge  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r28", "selfplay_cap.json")
POINTS = tuple((n, d) for n in (4096, 65536) for d in (0, 3))  # (boards, depth)
NOISE, SHARE, FAST = 64, 64, (16, 8)
ARRAYS = ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation", "visits", "value", "nodes", "how", "mover",
          "root_value", "priors", "outcomes", "proven")


class CapRunner(Runner):
    """Runner's position and arrays; the noised launch of this build and of a parent build, and the capped one."""

    def __init__(self, *args, parent=None, **kw):
        super().__init__(*args, **kw)
        self.parent_lib = parent

    def _args(self, a):
        e = C.addressof(self.struct)
        return (*self._head(a), nat.ptr(a["outcomes"]), nat.ptr(a["proven"]), self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T,
                nat.POLICY_EVAL_TREE, nat.POLICY_EVAL_TREE, e, e, self.I, self.I, self.depth, self.depth, NOISE, NOISE, X, 0, nat.ILLEGAL_NOOP,
                None, None)

    def noise(self):
        nat.check(nat.lib().gbl_collect_search_noise(*self._args(self.a), self.stream), "gbl_collect_search_noise")

    def parent(self):
        nat.check(self.parent_lib.gbl_collect_search_noise(*self._args(self.b), self.stream), "gbl_collect_search_noise (parent)")

    def cap(self, fast, share=SHARE):
        nat.check(nat.lib().gbl_collect_search_cap(*self._args(self.c), fast, fast, share, share, self.stream), "gbl_collect_search_cap")

    def cap16(self):
        self.cap(FAST[0])

    def cap8(self):
        self.cap(FAST[1])

    def check_same(self):
        """(p), (n) and the new entry point at shares (256, 256) write the same arrays."""
        n = self.n
        self.restore(); self.noise(); torch.cuda.synchronize()
        end = (self.st.clone(), self.tm.clone())
        self.restore(); self.cap(1, nat.CAP_FULL_SHARE); torch.cuda.synchronize()
        for k in ARRAYS:
            assert torch.equal(self.a[k][:, :n], self.c[k][:, :n]), k
        assert torch.equal(end[0], self.st) and torch.equal(end[1], self.tm)
        if self.parent_lib is not None:
            self.restore(); self.parent(); torch.cuda.synchronize()
            for k in ARRAYS:
                assert torch.equal(self.a[k][:, :n], self.b[k][:, :n]), k

    def census(self, arrays):
        """Of the window last written into `arrays`: kept rows, network evaluations, and the plies by kind."""
        n = self.n
        how = arrays["how"][:, :n]
        return {"kept_rows": int((arrays["visits"][:, :n].to(torch.int32).sum(-1) > 0).sum()),
                "evaluations": int(arrays["nodes"][:, :n].to(torch.int64).sum()),
                "full_plies": int(((how == nat.HOW_SEARCH) | (how == nat.HOW_SEARCH_SAMPLED)).sum()),
                "fast_plies": int((how >= nat.HOW_FAST).sum()), "proven_plies": int((how == nat.HOW_PROVEN).sum())}


def load_parent(path):
    L = C.CDLL(os.path.abspath(path))
    for name in ("gbl_collect_search_noise", "gbl_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L


def device(path, parent_path):
    parent = load_parent(parent_path) if parent_path else None
    names = (("parent",) if parent is not None else ()) + ("noise", "cap16", "cap8")
    rows, cache = [], {}
    for n, d in POINTS:
        if n not in cache:
            cache = {n: states(n)}
        r = CapRunner(*cache[n], I, seeded_evaluator(H), d, parent=parent)
        r.check_same()
        t = r.time(reps=REPS, names=names)
        r.restore(); r.noise(); torch.cuda.synchronize()
        full = r.census(r.a)
        base = t["parent"] if parent is not None else t["noise"]  # the uncapped window the ratios are taken against
        bm = stats(base)["median"]
        row = {"boards": n, "depth": d, "iterations": I, "hidden": H, "plies": T, "explore": X, "noise": NOISE, "full_share": SHARE,
               "uncapped_is": "parent build" if parent is not None else "this build (parent NOT MEASURED)",
               "noise_ms": stats(t["noise"]), "uncapped_census": full, "uncapped_kept_rows_per_s": full["kept_rows"] / (bm * 1e-3)}
        if parent is not None:
            p = stats(t["parent"])
            row.update(parent_ms=p, parent_spread_ms=p["max"] - p["min"], noise_over_parent=stats(t["noise"])["median"] / p["median"],
                       noise_within_parent_spread=within_spread(t["noise"], t["parent"]))
        else:
            row.update(parent_ms="NOT MEASURED")
        for name, fast in (("cap16", FAST[0]), ("cap8", FAST[1])):
            r.restore(); getattr(r, name)(); torch.cuda.synchronize()
            c, s = r.census(r.c), stats(t[name])
            row[name] = {"fast_iterations": fast, "ms": s, "over_uncapped": s["median"] / bm, "census": c,
                         "kept_rows_per_s": c["kept_rows"] / (s["median"] * 1e-3),
                         "evaluations_over_uncapped": c["evaluations"] / max(full["evaluations"], 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r
        torch.cuda.empty_cache()
        merge(path, "rows", rows)
    merge(path, "device", torch.cuda.get_device_name(0))
    merge(path, "method", "HIP events; evaluator against evaluator (seeded int8 weights, H %d, %d iterations, noise weight %d) from the same C5 "
          "position, state restored outside the timed region; one warm-up each, then %d repetitions alternating parent / noise / cap16 / "
          "cap8 in one process; ms per %d plies; parent = gbl_collect_search_noise of a library built from the parent commit; kept rows = "
          "cells with a non-zero visits row" % (H, I, NOISE, REPS, T))
    print("wrote", path)


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = args[i + 1]
        del args[i:i + 2]
    device(args[0] if args else DEFAULT_OUT, parent)


if __name__ == "__main__":
    main()
