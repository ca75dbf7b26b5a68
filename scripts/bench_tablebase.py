#!/usr/bin/env python3
"""The exact tablebase of the game's own inventory (2, 2, 2) on the GPU: the build, the probe against gbl_solve, the blunder census
against the true verdict, and the probe's time.  Four steps, each a process of its own (run each under its own `timeout`, chained with
&&); the build takes under a second, so every step builds its own table (2.9 GB of device memory) and nothing is written but the
record the steps merge their sections into:

    python scripts/bench_tablebase.py build   [out.json]    every sweep timed (wall clock around the sweep's launches and the one read
                                                            of its counter), the decided counts, the terminal count, the share of
                                                            draws, the value of the empty board
    python scripts/bench_tablebase.py compare [out.json]    the 4 096 masked-random states and the 4 096 self-play states of
                                                            scripts/bench_solver.py: all 54 bytes per board of the probe against
                                                            gbl_solve(depth = 4).  Exact: a probe result c with |c| <= 4 is the
                                                            solver's byte, |c| > 4 or c == 0 reads 0 there.  A mismatch FAILS.
    python scripts/bench_tablebase.py census  [out.json]    bench_solver.py's census of the four estimating policies on the same two
                                                            sets, against the table instead of the depth-4 verdict
    python scripts/bench_tablebase.py timing  [out.json]    gbl_tb_probe at 4 096 and 65 536 boards beside gbl_solve depth 2 and 4
                                                            (HIP events, one warm-up, the median of five)

Default record: profiles/r22/tablebase.json.  A smaller inventory for a dry run: GOBBLET_TB_INVENTORY=2,2,0 (its boards are not the
sets' boards: compare, census and timing need the full inventory)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_solver as B  # noqa: E402  (the two position sets, the example evaluator, the timing)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

DEV = B.DEV
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r22", "tablebase.json")
SLICE = 1 << 28   # positions per launch of the build: 11 launches per sweep of the full inventory
N = 4096


def build(path):
    inventory = tuple(int(c) for c in os.environ.get("GOBBLET_TB_INVENTORY", "2,2,2").split(","))
    tb = G.Tablebase(inventory, DEV)
    torch.cuda.synchronize()
    sweeps, t_all = [], time.perf_counter()
    while not tb.complete:
        t0 = time.perf_counter()
        tb.build(max_sweeps=1, slice_positions=SLICE)   # (reads the sweep's counter: the sweep has run when it returns)
        sweeps.append({"sweep": tb.sweeps - 1, "decided": tb.decided[-1], "seconds": time.perf_counter() - t0})
        print(json.dumps(sweeps[-1]), flush=True)
    total = time.perf_counter() - t_all
    draws = sum(int((tb.table[f:f + SLICE] == 0).sum()) for f in range(0, tb.positions, SLICE))
    rec = {"device": torch.cuda.get_device_name(0), "inventory": list(inventory), "positions": tb.positions, "bytes": tb.positions,
           "slice_positions": SLICE, "sweeps": sweeps, "sweeps_done": tb.sweeps, "last_deciding_sweep": tb.sweeps - 2,
           "total_seconds": total, "terminal_positions": tb.decided[0], "drawn_positions": draws, "share_of_draws": draws / tb.positions,
           "share_of_draws_among_non_terminal": draws / (tb.positions - tb.decided[0]), "value_of_the_empty_board": int(tb.value([0])[0]),
           "timing": "wall clock per sweep: its launches on one stream and the read of its device counter"}
    assert sum(tb.decided) + draws == tb.positions
    B.merge(path, "build", rec)


def full_table():
    tb = G.Tablebase((2, 2, 2), DEV)
    tb.build(slice_positions=SLICE)
    assert tb.complete
    return tb


def position_sets():
    return {"masked-random mix (seed 11, 64 plies)": lambda: B.states(N),
            "tree-against-tree self-play (TreeSearchGobbletPolicy(64, 16) both sides, boards after plies 6 / 10 / 14 / 18, seed 11)":
                lambda: B.selfplay_states(N, DEV)}


def compare(path):
    tb = full_table()
    recs = []
    for name, make in position_sets().items():
        st, tm = make()
        true = tb.probe(st, tm)["outcome"].cpu().numpy().astype(int)
        bounded = G.SolverGobbletPolicy(4, device=DEV).outcomes(st, tm).cpu().numpy().astype(int)
        expect = np.where((true != nat.SOLVE_NONE) & (np.abs(true) > 4), 0, true)
        bad = np.argwhere(expect != bounded)
        rec = {"positions": name, "boards": len(st), "bytes_compared": int(expect.size), "mismatches": int(len(bad)),
               "results_beyond_depth_4": int(((true != nat.SOLVE_NONE) & (np.abs(true) > 4)).sum()),
               "true_draws_among_actions": int((true == 0).sum()), "deepest_result": int(np.abs(np.where(true == nat.SOLVE_NONE, 0, true)).max())}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        if len(bad):
            B.merge(path, "compare_with_gbl_solve_depth_4", recs)
            raise SystemExit("the probe and gbl_solve(depth=4) differ at (board, action) %s" % bad[:5].tolist())
    B.merge(path, "compare_with_gbl_solve_depth_4", recs)


def census(path):
    tb = full_table()
    ev = B.example_evaluator(DEV)
    policies = {"GreedyGobbletPolicy(2)": lambda: G.GreedyGobbletPolicy(2, device=DEV),
                "TreeSearchGobbletPolicy(64, 16)": lambda: G.TreeSearchGobbletPolicy(64, 16, device=DEV),
                "TreeSearchGobbletPolicy(256, 16)": lambda: G.TreeSearchGobbletPolicy(256, 16, device=DEV),
                "EvaluatorTreeSearchGobbletPolicy(example network, 64)": lambda: G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=64, device=DEV)}
    recs = []
    for name, make in position_sets().items():
        st, tm = make()
        out = tb.probe(st, tm)["outcome"].cpu().numpy().astype(int)
        legal = out != nat.SOLVE_NONE
        has_win, has_draw = ((out > 0) & legal).any(1), (out == 0).any(1)
        rec = {"boards": len(st), "positions": name, "won_boards": int(has_win.sum()), "drawn_boards": int((~has_win & has_draw).sum()),
               "lost_boards": int((~has_win & ~has_draw & legal.any(1)).sum()), "policies": {}}
        for pname, pol in policies.items():
            a = pol().compute_actions_from_state(st, tm).cpu().numpy().astype(int)
            took = out[np.arange(len(st)), a]
            rec["policies"][pname] = {"missed_a_win": int((has_win & (took <= 0)).sum()),
                                      "turned_a_won_position_into_a_drawn_one": int((has_win & (took == 0)).sum()),
                                      "turned_a_won_position_into_a_lost_one": int((has_win & (took < 0)).sum()),
                                      "played_a_loss_with_a_drawing_move_at_hand": int((~has_win & has_draw & (took < 0)).sum())}
            print(name[:24], pname, rec["policies"][pname], flush=True)
        recs.append(rec)
    B.merge(path, "census_against_the_table", recs)


def timing(path):
    tb = full_table()
    rows = []
    for n in (4096, 65536):
        st, tm = B.states(n)
        row = {"boards": n, "gbl_tb_probe": B.timed(lambda: tb.probe(st, tm))}
        for depth in (2, 4):
            pol = G.SolverGobbletPolicy(depth, device=DEV)
            row["gbl_solve_depth_%d" % depth] = B.timed(lambda: pol.outcomes(st, tm))
        print(json.dumps(row), flush=True)
        rows.append(row)
    B.merge(path, "timing", {"method": "HIP events, one warm-up, five repetitions, the Python wrappers' allocations included on both sides",
                             "rows": rows})


if __name__ == "__main__":
    {"build": build, "compare": compare, "census": census, "timing": timing}[sys.argv[1]](sys.argv[2] if len(sys.argv) > 2 else DEFAULT_OUT)
