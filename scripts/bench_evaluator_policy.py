#!/usr/bin/env python3
"""gbl_tree_search_eval (EvaluatorTreeSearchGobbletPolicy) against its yardstick gbl_tree_search(iterations, 16 playouts) on the
same states in the same process, the two alternating; k_evaluate's evaluations per second; the `explore` sweep and the arena score
of the evaluator that examples/example_train_evaluator.py trains.

    python scripts/bench_evaluator_policy.py [out.json]         on the GPU (default: profiles/r10/evaluator_policy.json)
    python scripts/bench_evaluator_policy.py --host [out.json]  the sweep and the arena alone, on the host flavour
    python scripts/bench_evaluator_policy.py --timing [out.json]  the timing rows alone, on the GPU (the record's other sections stay)

States: the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE config 5).  HIP-event times, one
warm-up and 5 repetitions per point; the record keeps the median, and for the yardstick its minimum and maximum as well.  The
sweep's games are the same on either flavour of the library (the searches are integer-only), so it runs where the benchmark runs.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
import example_train_evaluator as EX  # noqa: E402

DEV = "cuda:0"
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r10", "evaluator_policy.json")
BOARDS, ITERATIONS, HIDDEN = (4096, 65536), (64, 256, 512), (64, 256)
SWEEP = (0, 16, 32, 64, 128, 256, 512)
REPS = 5


def random_evaluator(hidden, seed=0):
    rng = np.random.default_rng(seed)
    return G.GobbletEvaluator(rng.integers(-128, 128, (117, hidden), dtype=np.int8), rng.integers(-300, 300, hidden),
                              rng.integers(-128, 128, (hidden // 4, 56, 4), dtype=np.int8), rng.integers(-65536, 65536, 56), 1, 9, 9, device=DEV)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main(out_path, with_sweep=True):
    env = G.BatchedGobblet(max(BOARDS), DEV, auto_reset=True, seed=11)
    env.rollout(64)
    torch.cuda.synchronize()
    rows, evals = [], []
    for n in BOARDS:
        st, tm = env.squares[:n].clone(), env.to_move[:n].clone()
        for I in ITERATIONS:
            yard = G.TreeSearchGobbletPolicy(iterations=I, playouts=16, seed=0, device=DEV)
            pols = {h: G.EvaluatorTreeSearchGobbletPolicy(random_evaluator(h), iterations=I) for h in HIDDEN}
            for p in (yard, *pols.values()):  # warm-up
                p.compute_actions_from_state(st, tm)
            torch.cuda.synchronize()
            t_yard, t_eval = [], {h: [] for h in HIDDEN}
            for _ in range(REPS):  # alternating
                t_yard.append(event_ms(lambda: yard.compute_actions_from_state(st, tm)))
                for h in HIDDEN:
                    t_eval[h].append(event_ms(lambda: pols[h].compute_actions_from_state(st, tm)))
            y = float(np.median(t_yard))
            for h in HIDDEN:
                e = float(np.median(t_eval[h]))
                rows.append({"boards": n, "iterations": I, "hidden": h, "ms_per_launch": e, "ms_min": min(t_eval[h]), "ms_max": max(t_eval[h]),
                             "yardstick_ms": y, "yardstick_min_ms": min(t_yard),
                             "yardstick_max_ms": max(t_yard), "ratio_to_yardstick": e / y,
                             "leaves_per_s": float(pols[h].last_nodes.sum()) / (e * 1e-3)})
                print(rows[-1], flush=True)
        for h in HIDDEN:
            ev = random_evaluator(h)
            ev.evaluate_raw(st, tm)
            torch.cuda.synchronize()
            times = [event_ms(lambda: ev.evaluate_raw(st, tm)) for _ in range(REPS)]
            ms = float(np.median(times))
            evals.append({"boards": n, "hidden": h, "ms_per_launch": ms, "ms_min": min(times), "ms_max": max(times), "evaluations_per_s": n / (ms * 1e-3)})
            print(evals[-1], flush=True)
    rec = {"metric": "gbl_tree_search_eval vs gbl_tree_search(iterations, 16 playouts), HIP-event ms per launch (median of %d)" % REPS,
           "device": torch.cuda.get_device_name(0), "rows": rows, "k_evaluate": evals}
    merge(out_path, rec)  # (the timing is kept even if the games below are cut short)
    if with_sweep:
        merge(out_path, sweep(DEV, 256, (64, 256)))


def sweep(dev, games, arena_iterations):
    """Train the example's evaluator on `dev`, play every explore of SWEEP against the playout search at 64 iterations, then the best
    one at `arena_iterations`: the record's sections."""
    ev, samples, loss = EX.train_evaluator(dev)
    rows = []
    for x in SWEEP:
        w, l, d = EX.score(ev, dev, 64, games, explore=x)
        rows.append({"explore": x, "wins": w, "losses": l, "unfinished": d})
        print(rows[-1], flush=True)
    best = max(rows, key=lambda r: (r["wins"] - r["losses"], -r["explore"]))["explore"]
    arena = [dict(zip(("iterations", "wins", "losses", "unfinished"), (I, *EX.score(ev, dev, I, games, explore=best)))) for I in arena_iterations]
    print(arena, flush=True)
    return {"trained_evaluator": {"device": str(dev), "samples": samples, "final_loss": loss, "hidden": ev.hidden, "scales": ev.scales,
                                  "shifts": [ev.shift1, ev.shift_p, ev.shift_v]},
            "explore_sweep": {"opponent": "TreeSearchGobbletPolicy(iterations=64, playouts=16)", "iterations": 64, "games": games, "rows": rows},
            "explore_default": best, "arena_vs_playout_search": arena}


def merge(out_path, sections):
    rec = json.load(open(out_path)) if os.path.exists(out_path) else {}
    rec.update(sections)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(rec, open(out_path, "w"), indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a not in ("--host", "--timing")]
    if "--host" in sys.argv[1:]:  # the sweep and the arena alone, on the host flavour (fewer games: it is the CPU playing them)
        merge(args[0] if args else DEFAULT_OUT, sweep("cpu", 128, (64,)))
    else:
        main(args[0] if args else DEFAULT_OUT, with_sweep="--timing" not in sys.argv[1:])
