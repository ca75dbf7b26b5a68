#!/usr/bin/env python3
"""gbl_collect_gumbel_solve (solver-guarded Gumbel self-play): what the guard costs a 16-iteration window, in one process, on the stationary
masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE config 5), evaluator against evaluator with one seeded integer
network (H 64), Gumbel with 16 iterations and 16 considered actions, explore 16, T = 16.

    python scripts/bench_selfplay_gumbel_solve.py [out.json] [--parent lib.so]   on the GPU (default out: profiles/r32/selfplay_gumbel_solve.json)
    python scripts/bench_selfplay_gumbel_solve.py --host [out.json]              the arenas and the census on the host flavour (no GPU)

Per point (boards 4 096 / 65 536, depth 0 / 2 / 3), alternating, median of five with min - max:
  fused      ONE gbl_collect_gumbel_solve launch of T plies, both sides guarded at the depth (depth 0: the entry point without a guard,
             the guard's two arrays still written -- the same kernel with the solver never called);
  composed   per ply: gbl_solve (depth > 0); gbl_tree_search_gumbel(call = the ply index) on the WHOLE batch under the mask C = (outcome
             == 0) on the unproven boards and an empty row on the proven ones (the Gumbel row's board id is env_base + the row, so the
             sub-batch cannot be gathered: a proven board costs the loop one root evaluation); a torch pick between the solver's action
             and the rule's; gbl_step_into into slot t.  It plays the same games: its trajectory is compared with the fused one's before
             anything is timed;
  gumbel     ONE gbl_collect_search_gumbel launch (unguarded), of this build and (--parent) of a library built from the parent commit;
  solve      ONE gbl_collect_search_solve launch (PUCT, 64 iterations, guarded at the depth), of this build and (--parent) the parent's.
This build's `gumbel` and `solve` are held against the parent's min - max band.  Kept rows (cells with a non-zero visits row) per second
and the share of proven plies come from the fused window.  `guard`: 4 096 boards x depth 3 x 16 plies, fused against composed -- the row
tests/test_gpu_gumbel_solve_guard.py measures again.

--host: 256 games per colour on the seeded network on the host flavour (bit-identical to the kernels): guarded Gumbel-16 (depth 3)
against unguarded Gumbel-16 and against unguarded PUCT-64, and the blunder census of the guarded Gumbel ply against the verdict at the
guard's depth.  One seed: no claim beyond the table."""
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
from bench_gumbel import CONSIDERED, LARGE, OFFSET, SCALE, SMALL, WindowRunner  # noqa: E402
from bench_selfplay_eval import seeded_evaluator  # noqa: E402
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402
from bench_selfplay_solve import PLY0, H, X, first_games  # noqa: E402
from bench_solver import merge  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r32", "selfplay_gumbel_solve.json")
BOARDS, DEPTHS = (4096, 65536), (0, 2, 3)
SHARED = ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation", "visits", "nodes", "root_value", "priors",
          "outcomes", "proven")


def load_parent(path):
    L = C.CDLL(os.path.abspath(path))
    for name in ("gbl_collect_search_gumbel", "gbl_collect_search_solve", "gbl_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L


class GuardedRunner(WindowRunner):
    """bench_selfplay_solve's position and arrays (a: fused, b: composed, c: the unguarded and the PUCT windows)."""

    def __init__(self, st0, tm0, ev, depth, plies=T, parent=None):
        super().__init__(st0, tm0, SMALL, ev, depth, plies=plies, parent=parent)
        n, dev = self.n, st0.device
        z = lambda dt, *tail: torch.zeros((n,) + tail, dtype=dt, device=dev)  # noqa: E731
        self.tree = [z(torch.int32, 54), z(torch.int32, 54), z(torch.int32, 54), z(torch.int32), z(torch.int32), z(torch.int32), z(torch.uint8, 54)]
        self.target, self.mask, self.a_star = z(torch.uint8, 54), z(torch.int8, 54), z(torch.int32)
        self.hot = torch.arange(54, device=dev, dtype=torch.int32)[None]

    def _gumbel_tail(self):
        return (X, 0, nat.ILLEGAL_NOOP, None, None, CONSIDERED, CONSIDERED, 1, OFFSET, SCALE, self.stream)

    def fused(self):
        a = self.a
        nat.check(nat.lib().gbl_collect_gumbel_solve(*self._head(a), nat.ptr(a["outcomes"]), nat.ptr(a["proven"]), *self._tail(SMALL), self.depth,
                                                     self.depth, *self._gumbel_tail()), "gbl_collect_gumbel_solve")

    def composed(self):
        b, p, L, e, n = self.b, nat.ptr, nat.lib(), C.addressof(self.struct), self.n
        vis_, w_, l_, act_, nd_, rv_, pr_ = self.tree
        for t in range(self.T):
            out, V = b["outcomes"][t][:n], b["proven"][t][:n]
            mask = None
            if self.depth:
                nat.check(L.gbl_solve(p(self.st), p(self.tm), None, self.depth, p(out), p(V), p(self.a_star), n, self.stream), "gbl_solve")
                torch.logical_and(out == 0, (V == 0)[:, None], out=self.mask.view(torch.bool))
                mask = self.mask
            else:
                out.fill_(nat.SOLVE_NONE); V.zero_()
            nat.check(L.gbl_tree_search_gumbel(p(self.st), p(self.tm), p(mask), e, SMALL, X, CONSIDERED, 1, OFFSET, SCALE, self.seed, 0, PLY0 + t,
                                               p(vis_), p(w_), p(l_), p(act_), p(nd_), p(rv_), p(pr_), p(self.target), None, n, self.stream),
                      "gbl_tree_search_gumbel")
            if self.depth:  # the pick: the solver's action and its one-hot row on a proven board, the rule's elsewhere
                proven = V != 0
                torch.where(proven, self.a_star, act_, out=act_)
                b["visits"][t][:n] = torch.where(proven[:, None], (self.hot == self.a_star[:, None]).to(torch.int16) * SMALL, self.target.to(torch.int16))
                b["nodes"][t][:n] = torch.where(proven, 0, nd_)
                b["root_value"][t][:n] = torch.where(proven, 0, rv_)
                b["priors"][t][:n] = torch.where(proven[:, None], 0, pr_)
            else:
                b["visits"][t][:n] = self.target.to(torch.int16)
                b["nodes"][t][:n], b["root_value"][t][:n], b["priors"][t][:n] = nd_, rv_, pr_
            nat.check(L.gbl_step_into(p(self.st), p(self.tm), p(self.dn), p(act_), p(b["winner"][t]), p(b["rewards"][t]),
                                      p(b["action_mask"][t]), p(b["observation"][t]), None, p(b["actions"][t]), p(b["done"][t]),
                                      p(b["to_move"][t]), n, nat.ILLEGAL_NOOP, 1, self.stream), "gbl_step_into")

    def gumbel(self, lib=None):
        nat.check((lib or nat.lib()).gbl_collect_search_gumbel(*self._head(self.c), *self._tail(SMALL), *self._gumbel_tail()), "gbl_collect_search_gumbel")

    def solve(self, lib=None):
        c = self.c
        nat.check((lib or nat.lib()).gbl_collect_search_solve(*self._head(c), nat.ptr(c["outcomes"]), nat.ptr(c["proven"]), *self._tail(LARGE),
                                                              self.depth, self.depth, X, 0, nat.ILLEGAL_NOOP, None, None, self.stream),
                  "gbl_collect_search_solve")

    def parent_gumbel(self):
        self.gumbel(self.parent_lib)

    def parent_solve(self):
        self.solve(self.parent_lib)

    def check_equal(self):
        """fused and composed play the same games: every array they share, and the boards they end on."""
        self.restore(); self.fused(); torch.cuda.synchronize()
        end_a = (self.st.clone(), self.tm.clone(), self.dn.clone())
        self.restore(); self.composed(); torch.cuda.synchronize()
        n = self.n
        for k in SHARED:
            assert torch.equal(self.a[k][:, :n], self.b[k][:, :n]), k
        assert all(torch.equal(x, y) for x, y in zip(end_a, (self.st, self.tm, self.dn)))


def device(path, parent_path):
    parent = load_parent(parent_path) if parent_path else None
    ev = seeded_evaluator(H)
    rows = []
    for n in BOARDS:
        st, tm = states(n)
        for depth in DEPTHS:
            r = GuardedRunner(st, tm, ev, depth, parent=parent)
            r.check_equal()
            names = ("fused", "composed", "gumbel", "solve") + (("parent_gumbel", "parent_solve") if parent is not None else ())
            raw = r.time(reps=REPS, names=names)
            t = {k: stats(v) for k, v in raw.items()}
            r.restore(); r.fused(); torch.cuda.synchronize()
            kept = int((r.a["visits"][:, :n].to(torch.int32).sum(-1) > 0).sum())
            row = {"boards": n, "depth": depth, "plies": T, "hidden": H, "explore": X, "iterations": SMALL, "considered": CONSIDERED,
                   "puct_iterations": LARGE, "fused_ms": t["fused"], "composed_ms": t["composed"], "gumbel_ms": t["gumbel"], "solve_ms": t["solve"],
                   "fused_over_composed": t["fused"]["median"] / t["composed"]["median"],
                   "fused_over_unguarded_gumbel": t["fused"]["median"] / t["gumbel"]["median"],
                   "fused_over_guarded_puct": t["fused"]["median"] / t["solve"]["median"],
                   "proven_plies": float((r.a["proven"][:, :n] != 0).float().mean()), "kept_rows": kept,
                   "kept_rows_per_s": kept / (t["fused"]["median"] * 1e-3)}
            if parent is not None:
                row.update(parent_gumbel_ms=t["parent_gumbel"], parent_solve_ms=t["parent_solve"],
                           gumbel_within_parent_band=within_spread(raw["gumbel"], raw["parent_gumbel"]),
                           solve_within_parent_band=within_spread(raw["solve"], raw["parent_solve"]),
                           fused_over_parent_gumbel=t["fused"]["median"] / t["parent_gumbel"]["median"],
                           fused_over_parent_solve=t["fused"]["median"] / t["parent_solve"]["median"])
            else:
                row.update(parent_gumbel_ms="NOT MEASURED", parent_solve_ms="NOT MEASURED")
            print(json.dumps(row), flush=True)
            rows.append(row)
            if n == 4096 and depth == 3:
                merge(path, "guard", {"boards": n, "depth": depth, "plies": T, "fused_ms": t["fused"], "composed_ms": t["composed"],
                                      "fused_over_composed": row["fused_over_composed"]})
            del r
            torch.cuda.empty_cache()
            merge(path, "rows", rows)
    merge(path, "device", torch.cuda.get_device_name(0))
    merge(path, "method", "HIP events; evaluator against evaluator (seeded int8 weights, H %d) from the same C5 position, the state restored outside "
          "the timed region; one warm-up each, then %d repetitions alternating in one process; ms per %d plies; parent = a library built "
          "from the parent commit; kept rows = cells with a non-zero visits row" % (H, REPS, T))
    print("wrote", path)


def host(path, games=256, depth=3, plies=96):
    import bench_solver
    nat.cpu_raw().gbl_cpu_set_threads(16)
    ev = seeded_evaluator(H, "cpu")
    rule = dict(considered=CONSIDERED, visit_offset=OFFSET, scale=SCALE)
    arena = []
    # the guarded Gumbel-16 side as player_1, then as player_2; the other side unguarded Gumbel-16, then unguarded PUCT-64
    for other, other_its, other_considered in (("unguarded Gumbel-%d" % SMALL, SMALL, CONSIDERED), ("unguarded PUCT-%d" % LARGE, LARGE, 0)):
        for guarded in (0, 1):
            t0 = time.perf_counter()
            its, cons, deps = [other_its] * 2, [other_considered] * 2, [0, 0]
            its[guarded], cons[guarded], deps[guarded] = SMALL, CONSIDERED, depth
            env = G.BatchedGobblet(games, "cpu", auto_reset=True, seed=11, track_turn=True)
            tr = env.collect(plies, policies=("evaluator", "evaluator"),
                             search=dict(evaluator=ev, iterations=tuple(its), explore=X, sample_plies=4,
                                         gumbel=dict(rule, considered=tuple(cons), solve_depth=tuple(deps))))
            win, finished = first_games(tr)
            mine = 1 if guarded == 0 else -1
            arena.append({"guarded_side": "player_%d" % (guarded + 1), "against": other, "games": games,
                          "finished_within_%d_plies" % plies: int(finished.sum()), "guarded_wins": int((win == mine).sum()),
                          "other_wins": int((win == -mine).sum()), "proven_plies": int((tr["how"].numpy() == nat.HOW_PROVEN).sum()),
                          "seconds": time.perf_counter() - t0})
            print(arena[-1], flush=True)
    merge(path, "arena_host_flavour", {"network": "seeded int8 weights, H %d (untrained)" % H, "guarded": "Gumbel-%d, depth %d" % (SMALL, depth),
                                       "gumbel": rule, "sample_plies": "4 (read by the PUCT side alone)", "rows": arena,
                                       "note": "one seed: no claim beyond the table"})
    recs = []
    sets = {"masked-random mix (seed 11, 64 plies)": lambda: bench_solver.states(4096, "cpu"),
            "tree-against-tree self-play (TreeSearchGobbletPolicy(64, 16) both sides, boards after plies 6 / 10 / 14 / 18, seed 11)":
                lambda: bench_solver.selfplay_states(4096, "cpu")}
    for positions, make in sets.items():
        st, tm = make()
        env = G.BatchedGobblet(len(st), "cpu", auto_reset=True, seed=11)
        env.squares.copy_(st); env.to_move.copy_(tm)
        tr = env.collect(1, policies=("evaluator", "evaluator"), refresh=False,
                         search=dict(evaluator=ev, iterations=SMALL, explore=X, gumbel=dict(rule, solve_depth=depth)))
        a = tr["actions"][0].numpy().astype(int)
        out = G.SolverGobbletPolicy(depth, device="cpu").outcomes(st, tm).numpy().astype(int)
        legal = out != nat.SOLVE_NONE
        has_win, has_open = ((out > 0) & legal).any(1), (out == 0).any(1)
        took = out[np.arange(len(st)), a]
        rec = {"boards": len(st), "positions": positions, "guard_depth": depth,
               "boards_with_a_proven_win": int(has_win.sum()),
               "boards_with_a_proven_loss_and_an_unproven_move": int(((out < 0) & legal).any(1)[has_open & ~has_win].sum()),
               "missed_a_proven_win": int((has_win & (took <= 0)).sum()),
               "played_a_proven_loss_with_an_unproven_move_at_hand": int((~has_win & has_open & (took < 0)).sum())}
        print(rec, flush=True)
        recs.append(rec)
    merge(path, "census_guarded_host_flavour", recs)
    print("wrote", path)


def main():
    args = sys.argv[1:]
    parent, on_host = None, "--host" in args
    if on_host:
        args.remove("--host")
    if "--parent" in args:
        i = args.index("--parent")
        parent = args[i + 1]
        del args[i:i + 2]
    path = args[0] if args else DEFAULT_OUT
    if on_host:
        host(path)
    else:
        device(path, parent)


if __name__ == "__main__":
    main()
