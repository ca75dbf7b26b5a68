#!/usr/bin/env python3
"""gbl_collect_search_solve (solver-guarded evaluator self-play): the fused launch against the composed device loop and against the
unguarded launch, in the same process, on the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE
config 5), evaluator against evaluator with one seeded integer network (H 64), 64 iterations, explore 16, sample_plies 0, T = 16.

    python scripts/bench_selfplay_solve.py [out.json] [--points N,D ...]   on the GPU (default: profiles/r16/selfplay_solve.json)
    python scripts/bench_selfplay_solve.py --host [out.json]               the arena and the census on the host flavour (no GPU)

  (a) fused      ONE gbl_collect_search_solve launch of T plies, both sides guarded at depth D;
  (b) composed   per ply: gbl_solve; the boards with V == 0 gathered (a nonzero: one host sync), gbl_tree_search_eval on the sub-batch
                 under the mask C = (outcome == 0), the actions scattered back; gbl_step_into into slot t of the trajectory arrays;
  (c) unguarded  ONE gbl_collect_search_eval launch of T plies: (a) - (c) is the price of the guard.
(a) and (b) start every repetition from the same position and play the same games: (b)'s trajectory is compared with (a)'s before
anything is timed.  Method: HIP events, one warm-up each, then REPS repetitions alternating (a), (b), (c); median, min and max.
`guard`: 4 096 boards x depth 3 x 8 plies, the row tests/test_gpu_selfplay_solve.py holds.  `solve_depth4_4096`: gbl_solve alone,
4 096 boards at depth 4 (k_solve shares its three phases with the fused kernel).

--host: an arena on the host flavour (bit-identical to the kernels), the guarded side (depth 3) against the unguarded one with the
same network and 64 iterations, both colours, 256 games each, the first 4 plies of every game drawn from the visits; and the blunder
census of scripts/bench_solver.py for the guarded policy (one guarded ply of the fused entry point from each of the census's two
position sets, against the solver's verdict at the guard's depth, where it must read 0 / 0, and at depth 4)."""
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
from bench_selfplay_eval import seeded_evaluator  # noqa: E402,F401
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402,F401
from bench_solver import merge  # noqa: E402

DEV = "cuda:0"
X, I, H = 16, 64, 64
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r16", "selfplay_solve.json")
POINTS = tuple((n, d) for n in (4096, 65536) for d in (2, 3))  # (boards, depth)
PLY0 = 100
SHARED = ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation", "nodes", "root_value", "priors", "outcomes",
          "proven")


class Runner:
    """One position, three ways to play T plies of evaluator against evaluator from it into trajectory arrays of one's own."""

    def __init__(self, st0, tm0, iterations, ev, depth, plies=T, seed=0):
        self.n, self.I, self.T, self.seed, self.ev, self.depth = st0.shape[0], iterations, plies, seed, ev, depth
        self.st0, self.tm0 = st0, tm0
        n, dev = self.n, st0.device
        self.slot = -(-n // 128) * 128
        self.st, self.tm, self.dn = st0.clone(), tm0.clone(), torch.zeros(n, dtype=torch.int8, device=dev)
        z = lambda dt, *tail: torch.zeros((plies, self.slot) + tail, dtype=dt, device=dev)  # noqa: E731

        def arrays():
            return dict(actions=z(torch.int32), winner=z(torch.int8), rewards=z(torch.int8, 2), done=z(torch.int8), to_move=z(torch.int8),
                        action_mask=z(torch.int8, 54), observation=z(torch.int8, 117), visits=z(torch.int16, 54), nodes=z(torch.int32),
                        root_value=z(torch.int32), priors=z(torch.uint8, 54), value=z(torch.int32), how=z(torch.int8), mover=z(torch.int8),
                        outcomes=z(torch.int8, 54), proven=z(torch.int8))
        self.a, self.b, self.c = arrays(), arrays(), arrays()
        self.b.update(act=torch.zeros(n, dtype=torch.int32, device=dev))
        self.stream = nat.current_stream(dev)
        self.struct = ev.as_struct()

    def restore(self):
        self.st.copy_(self.st0); self.tm.copy_(self.tm0); self.dn.zero_()

    def _head(self, a):
        p = nat.ptr
        return (p(self.st), p(self.tm), p(self.dn), p(a["actions"]), p(a["winner"]), p(a["rewards"]), p(a["done"]), p(a["to_move"]),
                p(a["action_mask"]), p(a["observation"]), p(a["visits"]), p(a["value"]), p(a["nodes"]), p(a["how"]), p(a["mover"]),
                p(a["root_value"]), p(a["priors"]))

    def fused(self):
        a, e = self.a, C.addressof(self.struct)
        nat.check(nat.lib().gbl_collect_search_solve(
            *self._head(a), nat.ptr(a["outcomes"]), nat.ptr(a["proven"]), self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T,
            nat.POLICY_EVAL_TREE, nat.POLICY_EVAL_TREE, e, e, self.I, self.I, self.depth, self.depth, X, 0, nat.ILLEGAL_NOOP, None, None,
            self.stream), "gbl_collect_search_solve")

    def unguarded(self):
        e = C.addressof(self.struct)
        nat.check(nat.lib().gbl_collect_search_eval(
            *self._head(self.c), self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T, nat.POLICY_EVAL_TREE, nat.POLICY_EVAL_TREE, e, e,
            self.I, self.I, X, 0, nat.ILLEGAL_NOOP, None, None, self.stream), "gbl_collect_search_eval")

    def composed(self):
        b, p, L, e, n = self.b, nat.ptr, nat.lib(), C.addressof(self.struct), self.n
        for t in range(self.T):
            out, V = b["outcomes"][t][:n], b["proven"][t][:n]
            nat.check(L.gbl_solve(p(self.st), p(self.tm), None, self.depth, p(out), p(V), p(b["act"]), n, self.stream), "gbl_solve")
            idx = torch.nonzero(V == 0)[:, 0]  # (the host learns the sub-batch's size here)
            k = int(idx.numel())
            vis = torch.zeros((n, 54), dtype=torch.int32, device=out.device)
            nodes, rootv = b["nodes"][t][:n].zero_(), b["root_value"][t][:n].zero_()
            pri = b["priors"][t][:n].zero_()
            if k:
                st, tm, mask = self.st[idx].contiguous(), self.tm[idx].contiguous(), (out[idx] == 0).to(torch.int8).contiguous()
                v, w, l = (torch.empty((k, 54), dtype=torch.int32, device=out.device) for _ in range(3))
                a, nd, rv = (torch.empty(k, dtype=torch.int32, device=out.device) for _ in range(3))
                pr = torch.empty((k, 54), dtype=torch.uint8, device=out.device)
                nat.check(L.gbl_tree_search_eval(p(st), p(tm), p(mask), e, self.I, X, p(v), p(w), p(l), p(a), p(nd), p(rv), p(pr), k,
                                                 self.stream), "gbl_tree_search_eval")
                b["act"][idx], vis[idx], nodes[idx], rootv[idx], pri[idx] = a, v, nd, rv, pr
            b["visits"][t][:n] = vis.to(torch.int16)
            nat.check(L.gbl_step_into(p(self.st), p(self.tm), p(self.dn), p(b["act"]), p(b["winner"][t]), p(b["rewards"][t]),
                                      p(b["action_mask"][t]), p(b["observation"][t]), None, p(b["actions"][t]), p(b["done"][t]),
                                      p(b["to_move"][t]), n, nat.ILLEGAL_NOOP, 1, self.stream), "gbl_step_into")

    def check_equal(self):
        """(a) and (b) play the same games: every array they share (a proven ply's one-hot row is (a)'s own)."""
        self.restore(); self.fused(); torch.cuda.synchronize()
        end_a = (self.st.clone(), self.tm.clone(), self.dn.clone())
        self.restore(); self.composed(); torch.cuda.synchronize()
        n = self.n
        for k in SHARED:
            assert torch.equal(self.a[k][:, :n], self.b[k][:, :n]), k
        searched = (self.a["proven"][:, :n] == 0)
        assert torch.equal(self.a["visits"][:, :n][searched], self.b["visits"][:, :n][searched])
        assert torch.equal(self.a["how"][:, :n] == nat.HOW_PROVEN, ~searched)
        assert all(torch.equal(x, y) for x, y in zip(end_a, (self.st, self.tm, self.dn)))

    def time(self, reps=REPS, names=("fused", "composed", "unguarded")):
        """{name: [ms]}: alternating, after a warm-up of each."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = {k: [] for k in names}
        for rep in range(reps + 1):
            for name in names:
                self.restore()
                torch.cuda.synchronize()
                e0.record()
                getattr(self, name)()
                e1.record()
                torch.cuda.synchronize()
                if rep:  # (repetition 0 is the warm-up)
                    out[name].append(e0.elapsed_time(e1))
        return out


def device(path, points):
    import bench_solver
    rows, cache = [], {}
    for n, d in points:
        if n not in cache:
            cache = {n: states(n)}
        r = Runner(*cache[n], I, seeded_evaluator(H), d)
        r.check_equal()
        t = r.time()
        proven = float((r.a["proven"][:, :n] != 0).float().mean())
        row = {"boards": n, "depth": d, "iterations": I, "hidden": H, "plies": T, "explore": X, "fused_ms": stats(t["fused"]),
               "composed_ms": stats(t["composed"]), "unguarded_ms": stats(t["unguarded"]), "proven_plies": proven,
               "fused_over_composed": stats(t["fused"])["median"] / stats(t["composed"])["median"],
               "fused_minus_unguarded_ms": stats(t["fused"])["median"] - stats(t["unguarded"])["median"],
               "within_spread": within_spread(t["fused"], t["composed"])}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r
        torch.cuda.empty_cache()
        merge(path, "rows", rows)
    r = Runner(*states(4096), I, seeded_evaluator(H), 3, plies=8)
    r.check_equal()
    t = r.time()
    merge(path, "guard", {"boards": 4096, "depth": 3, "plies": 8, "iterations": I, "hidden": H, "fused_ms": stats(t["fused"]),
                          "composed_ms": stats(t["composed"]), "unguarded_ms": stats(t["unguarded"])})
    print("guard", stats(t["fused"]), stats(t["composed"]), flush=True)
    st, tm = states(4096)
    out, val = torch.empty((4096, 54), dtype=torch.int8, device=DEV), torch.empty(4096, dtype=torch.int8, device=DEV)
    act = torch.empty(4096, dtype=torch.int32, device=DEV)
    s4 = bench_solver.timed(lambda: nat.check(nat.lib().gbl_solve(st.data_ptr(), tm.data_ptr(), None, 4, out.data_ptr(), val.data_ptr(),
                                                                  act.data_ptr(), 4096, nat.current_stream(DEV)), "gbl_solve"))
    merge(path, "solve_depth4_4096", s4)
    merge(path, "device", torch.cuda.get_device_name(0))
    merge(path, "method", "HIP events; evaluator against evaluator (seeded int8 weights, H %d, %d iterations) from the same C5 position, state "
          "restored outside the timed region; one warm-up each, then %d repetitions alternating fused / composed / unguarded; ms per "
          "`plies` plies" % (H, I, REPS))
    print("solve depth 4, 4096 boards", s4, "\nwrote", path)


def first_games(traj):
    """Per board the winner of its first finished game in the window (0: none finished, or a draw by an illegal move)."""
    done, win = traj["done"].numpy() != 0, traj["winner"].numpy()
    first = done.argmax(0)
    return np.where(done.any(0), win[first, np.arange(done.shape[1])], 0), done.any(0)


def host(path, games=256, depth=3, plies=96):
    import bench_solver
    nat.cpu_raw().gbl_cpu_set_threads(16)
    ev = seeded_evaluator(H, "cpu")
    arena = []
    for deps in ((depth, 0), (0, depth)):
        t0 = time.perf_counter()
        env = G.BatchedGobblet(games, "cpu", auto_reset=True, seed=11, track_turn=True)
        tr = env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=I, explore=X, sample_plies=4,
                                                                                 solve_depth=deps))
        win, finished = first_games(tr)
        guarded_is = 1 if deps[0] else -1
        arena.append({"solve_depth": list(deps), "games": games, "finished_within_%d_plies" % plies: int(finished.sum()),
                      "guarded_wins": int((win == guarded_is).sum()), "unguarded_wins": int((win == -guarded_is).sum()),
                      "proven_plies": int((tr["how"].numpy() == nat.HOW_PROVEN).sum()), "seconds": time.perf_counter() - t0})
        print(arena[-1], flush=True)
    merge(path, "arena_host_flavour", {"network": "seeded int8 weights, H %d (untrained)" % H, "iterations": I, "sample_plies": 4,
                                       "rows": arena})
    recs = []
    sets = {"masked-random mix (seed 11, 64 plies)": lambda: bench_solver.states(4096, "cpu"),
            "tree-against-tree self-play (TreeSearchGobbletPolicy(64, 16) both sides, boards after plies 6 / 10 / 14 / 18, seed 11)":
                lambda: bench_solver.selfplay_states(4096, "cpu")}
    for positions, make in sets.items():
        st, tm = make()
        env = G.BatchedGobblet(len(st), "cpu", auto_reset=True, seed=11)
        env.squares.copy_(st); env.to_move.copy_(tm)
        tr = env.collect(1, policies=("evaluator", "evaluator"), refresh=False,
                         search=dict(evaluator=ev, iterations=I, explore=X, solve_depth=depth))
        a = tr["actions"][0].numpy().astype(int)
        rec = {"boards": len(st), "positions": positions, "guard_depth": depth, "verdicts": {}}
        for d in sorted({2, depth, 4}):
            out = G.SolverGobbletPolicy(d, device="cpu").outcomes(st, tm).numpy().astype(int)
            legal = out != nat.SOLVE_NONE
            has_win, has_open = ((out > 0) & legal).any(1), (out == 0).any(1)
            took = out[np.arange(len(st)), a]
            rec["verdicts"]["depth %d" % d] = {
                "boards_with_a_proven_win": int(has_win.sum()),
                "boards_with_a_proven_loss_and_an_unproven_move": int(((out < 0) & legal).any(1)[has_open & ~has_win].sum()),
                "missed_a_proven_win": int((has_win & (took <= 0)).sum()),
                "played_a_proven_loss_with_an_unproven_move_at_hand": int((~has_win & has_open & (took < 0)).sum())}
            if d <= depth:
                v = rec["verdicts"]["depth %d" % d]
                assert v["missed_a_proven_win"] == 0 and v["played_a_proven_loss_with_an_unproven_move_at_hand"] == 0, v
        print(rec, flush=True)
        recs.append(rec)
    merge(path, "census_guarded_host_flavour", recs)


def main():
    args = sys.argv[1:]
    is_host = "--host" in args
    args = [a for a in args if a != "--host"]
    points = POINTS
    if "--points" in args:
        i = args.index("--points")
        points = tuple(tuple(int(x) for x in a.split(",")) for a in args[i + 1:])
        args = args[:i]
    path = args[0] if args else DEFAULT_OUT
    (host if is_host else device)(path, *(() if is_host else (points,)))


if __name__ == "__main__":
    main()
