#!/usr/bin/env python3
"""gbl_solve (SolverGobbletPolicy): time per launch on the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as
BASELINE config 5), and a blunder census of the estimating policies against the depth-4 verdict.

    python scripts/bench_solver.py [out.json]          timing on the GPU (default: profiles/r14/solver.json)
    python scripts/bench_solver.py --host [out.json]   the census on the host flavour (bit-identical to the kernels: no GPU needed)

Both modes merge their sections into the same record.  Timing: HIP events, one warm-up, five repetitions, min / median / max; beside
each row the host flavour on 16 threads (on the first HOST_BOARDS boards where the whole batch would take minutes: host_boards says
how many) and, at depth 2, gbl_greedy(depth=2) on the same boards.  A row whose launch would outlast the budget (estimated from the row
before it) is recorded as NOT MEASURED.  GOBBLET_HIP_LIB=build/lib_NAME.so times an experiment build (scripts/build_variant.sh).
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

if os.environ.get("GOBBLET_HIP_LIB"):
    nat.use_library(os.environ["GOBBLET_HIP_LIB"])

DEV = "cuda:0"
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r14", "solver.json")
ROWS = [(4096, d) for d in (1, 2, 3, 4, 5)] + [(65536, d) for d in (1, 2, 3, 4)]
HOST_BOARDS = {4: 2048, 5: 128}  # depth -> boards the host flavour is timed on (the first of the batch)
LAUNCH_BUDGET_MS = 60e3            # a row is skipped when its launch is estimated (x 30 per ply) to take longer


def states(n, dev=DEV):
    env = G.BatchedGobblet(n, dev, auto_reset=True, seed=11)
    env.rollout(64)
    if dev != "cpu":
        torch.cuda.synchronize()
    return env.squares.clone(), env.to_move.clone()


def timed(fn, iters=5):
    fn()  # warm
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return {"min_ms": min(times), "median_ms": float(np.median(times)), "max_ms": max(times)}


def merge(path, section, value):
    rec = {}
    if os.path.exists(path):
        with open(path) as f:
            rec = json.load(f)
    rec[section] = value
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def timing(path):
    cpu = nat.cpu_raw()
    cpu.gbl_cpu_set_threads(16)
    rows, last = [], {}
    for n, depth in ROWS:
        st, tm = states(n)
        out = torch.empty((n, 54), dtype=torch.int8, device=DEV)
        val = torch.empty(n, dtype=torch.int8, device=DEV)
        act = torch.empty(n, dtype=torch.int32, device=DEV)
        row = {"boards": n, "depth": depth}
        if last.get(n, 0) * 30 > LAUNCH_BUDGET_MS:
            row["device"] = "NOT MEASURED (estimated beyond the launch budget of this script)"
            rows.append(row)
            continue

        def go():
            nat.check(nat.lib().gbl_solve(st.data_ptr(), tm.data_ptr(), None, depth, out.data_ptr(), val.data_ptr(), act.data_ptr(), n,
                                          nat.current_stream(DEV)), "gbl_solve")
        row["device"] = timed(go)
        last[n] = row["device"]["median_ms"]
        row["boards_per_s"] = n / (row["device"]["median_ms"] * 1e-3)
        v = val.cpu().numpy()
        row["proven_roots"] = float((v != 0).mean())
        hn = min(n, HOST_BOARDS.get(depth, n))
        hs, hm = st[:hn].cpu().numpy().copy(), tm[:hn].cpu().numpy().copy()
        ho, hv, ha = np.empty((hn, 54), np.int8), np.empty(hn, np.int8), np.empty(hn, np.int32)
        t0 = time.perf_counter()
        assert cpu.gbl_cpu_solve(hs.ctypes.data, hm.ctypes.data, None, depth, ho.ctypes.data, hv.ctypes.data, ha.ctypes.data, hn, None) == 0
        row["host_16_threads_ms"], row["host_boards"] = (time.perf_counter() - t0) * 1e3, hn
        assert np.array_equal(ho, out[:hn].cpu().numpy()) and np.array_equal(ha, act[:hn].cpu().numpy())
        if depth == 2:
            cm, fb = torch.empty((n, 54), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)

            def greedy():
                nat.check(nat.lib().gbl_greedy(st.data_ptr(), tm.data_ptr(), None, None, 2, act.data_ptr(), cm.data_ptr(), fb.data_ptr(), n,
                                               nat.current_stream(DEV)), "gbl_greedy")
            row["gbl_greedy_depth_2"] = timed(greedy)
        print(json.dumps(row), flush=True)
        rows.append(row)
        merge(path, "timing_" + os.path.basename(nat.LIB_PATH), rows)


def selfplay_states(n, dev, iterations=64, playouts=16, plies=(6, 10, 14, 18)):
    """n boards of tree-against-tree self-play: TreeSearchGobbletPolicy(iterations, playouts) on both sides of n / len(plies) boards
    with auto-reset, the boards copied after each ply of `plies` (a finished game restarts in place, so the copies hold openings too,
    and no board with a winner)."""
    per = n // len(plies)
    env = G.BatchedGobblet(per, dev, auto_reset=True, seed=11)
    pol = G.TreeSearchGobbletPolicy(iterations, playouts, seed=11, device=dev)
    st, tm = [], []
    for t in range(1, max(plies) + 1):
        env.step(pol.compute_actions_from_state(env.squares, env.to_move, env.action_mask))
        if t in plies:
            st.append(env.squares.clone())
            tm.append(env.to_move.clone())
    return torch.cat(st), torch.cat(tm)


def example_evaluator(dev):
    """The network of examples/example_train_evaluator.py at its defaults: 512 boards x 48 plies of tree-against-tree self-play, 400
    Adam steps on a 117-64-55 MLP, quantised."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import example_train_evaluator as ex
    return ex.train_evaluator(dev)[0]


def census(path, n=4096, dev="cpu"):
    """On n boards of the masked-random mix and n of tree-against-tree self-play: how often a policy passes over a proven win (the
    depth-4 solver knows a winning action, the policy's is not one) and how often it plays a proven loss although an unproven action
    existed."""
    nat.cpu_raw().gbl_cpu_set_threads(16)
    t0 = time.perf_counter()
    ev = example_evaluator(dev)
    print("example evaluator trained in %.1f s" % (time.perf_counter() - t0), flush=True)
    policies = {"GreedyGobbletPolicy(2)": lambda: G.GreedyGobbletPolicy(2, device=dev),  # (fresh per set: greedy keeps a history)
                "TreeSearchGobbletPolicy(64, 16)": lambda: G.TreeSearchGobbletPolicy(64, 16, device=dev),
                "TreeSearchGobbletPolicy(256, 16)": lambda: G.TreeSearchGobbletPolicy(256, 16, device=dev),
                "EvaluatorTreeSearchGobbletPolicy(example network, 64)": lambda: G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=64, device=dev)}
    sets = {"masked-random mix (seed 11, 64 plies)": lambda: states(n, dev),
            "tree-against-tree self-play (TreeSearchGobbletPolicy(64, 16) both sides, boards after plies 6 / 10 / 14 / 18, seed 11)":
                lambda: selfplay_states(n, dev)}
    recs = []
    for positions, make in sets.items():
        st, tm = make()
        out = G.SolverGobbletPolicy(4, device=dev).outcomes(st, tm).cpu().numpy().astype(int)
        legal = out != nat.SOLVE_NONE
        has_win = ((out > 0) & legal).any(1)
        has_open = (out == 0).any(1)
        rec = {"boards": len(st), "device": dev, "positions": positions, "boards_with_a_proven_win": int(has_win.sum()),
               "boards_with_a_proven_loss_and_an_unproven_move": int(((out < 0) & legal).any(1)[has_open & ~has_win].sum()), "policies": {}}
        for name, pol in policies.items():
            t0 = time.perf_counter()
            a = pol().compute_actions_from_state(st, tm).cpu().numpy().astype(int)
            took = out[np.arange(len(st)), a]
            rec["policies"][name] = {"missed_a_proven_win": int((has_win & (took <= 0)).sum()),
                                     "played_a_proven_loss_with_an_unproven_move_at_hand": int((~has_win & has_open & (took < 0)).sum()),
                                     "seconds": time.perf_counter() - t0}
            print(positions[:24], name, rec["policies"][name], flush=True)
        recs.append(rec)
    merge(path, "census", recs)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = args[0] if args else DEFAULT_OUT
    if "--host" in sys.argv:
        census(path)
    else:
        timing(path)
