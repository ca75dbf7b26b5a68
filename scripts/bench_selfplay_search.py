#!/usr/bin/env python3
"""gbl_collect_search (search-driven self-play collection): the fused launch against the composed loop on the entry points that
existed before it, in the same process, on the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE
config 5), tree against tree, max_plies 64, explore 16, T = 16 plies.

    python scripts/bench_selfplay_search.py [out.json]     on the GPU (default: profiles/r09/selfplay_search.json)
    python scripts/bench_selfplay_search.py --trace N I P  one warm launch + 2 timed ones of the fused kernel, for rocprofv3 runs

  (a) fused     ONE gbl_collect_search launch of T plies;
  (b) composed  per ply: gbl_tree_search(call = q) into slot t of visits / wins / losses / nodes arrays, then gbl_step_into with
                the search's action_out into slot t of the seven trajectory arrays -- 2 T launches and the action's round trip.
Both start every repetition from the same position and ply index (the state is restored outside the timed region), so they play
the same games: (b)'s trajectory is compared with (a)'s before anything is timed.  Method: HIP events around the launch / the
loop, one warm-up each, then REPS repetitions alternating (a) and (b); the record keeps median, min and max.  The expectation
(a) <= (b) is judged against (b)'s own min-to-max spread of the run: `within_spread` = median(a) <= median(b) + (max(b) - min(b)).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

DEV = "cuda:0"
M, X, T, REPS = 64, 16, 16, 5
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r09", "selfplay_search.json")
POINTS = ((4096, 64, 16), (4096, 256, 16), (65536, 64, 16), (65536, 256, 16))  # (boards, iterations, playouts)
PLY0 = 100


def states(n, dev=DEV):
    env = G.BatchedGobblet(n, dev, auto_reset=True, seed=11)
    env.rollout(64)
    torch.cuda.synchronize()
    return env.squares.clone(), env.to_move.clone()


class Runner:
    """One position, two ways to play T plies of tree against tree from it into trajectory arrays of one's own."""

    def __init__(self, st0, tm0, I, P, plies=T, seed=0):
        self.n, self.I, self.P, self.T, self.seed = st0.shape[0], I, P, plies, seed
        self.st0, self.tm0 = st0, tm0
        n, dev = self.n, st0.device
        self.slot = -(-n // 128) * 128
        self.st, self.tm, self.dn = st0.clone(), tm0.clone(), torch.zeros(n, dtype=torch.int8, device=dev)

        def arrays(visit_dtype):
            z = lambda dt, *tail: torch.zeros((plies, self.slot) + tail, dtype=dt, device=dev)  # noqa: E731
            return dict(actions=z(torch.int32), winner=z(torch.int8), rewards=z(torch.int8, 2), done=z(torch.int8), to_move=z(torch.int8),
                        action_mask=z(torch.int8, 54), observation=z(torch.int8, 117), visits=z(visit_dtype, 54), nodes=z(torch.int32))
        self.a = arrays(torch.int16)
        self.a.update(value=torch.zeros((plies, self.slot), dtype=torch.int32, device=dev),
                      how=torch.zeros((plies, self.slot), dtype=torch.int8, device=dev),
                      mover=torch.zeros((plies, self.slot), dtype=torch.int8, device=dev))
        self.b = arrays(torch.int32)
        self.b.update(wins=torch.zeros_like(self.b["visits"]), losses=torch.zeros_like(self.b["visits"]),
                      act=torch.zeros(n, dtype=torch.int32, device=dev))
        self.stream = nat.current_stream(dev)

    def restore(self):
        self.st.copy_(self.st0); self.tm.copy_(self.tm0); self.dn.zero_()

    def fused(self):
        a, p = self.a, nat.ptr
        nat.check(nat.lib().gbl_collect_search(
            p(self.st), p(self.tm), p(self.dn), p(a["actions"]), p(a["winner"]), p(a["rewards"]), p(a["done"]), p(a["to_move"]),
            p(a["action_mask"]), p(a["observation"]), p(a["visits"]), p(a["value"]), p(a["nodes"]), p(a["how"]), p(a["mover"]), self.n,
            self.slot, 64, self.seed, 0, PLY0, None, self.T, nat.POLICY_TREE, nat.POLICY_TREE, self.I, self.I, self.P, self.P, M, X, 0,
            nat.ILLEGAL_NOOP, None, None, self.stream), "gbl_collect_search")

    def composed(self):
        b, p, L = self.b, nat.ptr, nat.lib()
        for t in range(self.T):
            nat.check(L.gbl_tree_search(p(self.st), p(self.tm), None, self.I, self.P, M, X, self.seed, 0, PLY0 + t, p(b["visits"][t]),
                                        p(b["wins"][t]), p(b["losses"][t]), p(b["act"]), p(b["nodes"][t]), None, self.n, self.stream),
                      "gbl_tree_search")
            nat.check(L.gbl_step_into(p(self.st), p(self.tm), p(self.dn), p(b["act"]), p(b["winner"][t]), p(b["rewards"][t]),
                                      p(b["action_mask"][t]), p(b["observation"][t]), None, p(b["actions"][t]), p(b["done"][t]),
                                      p(b["to_move"][t]), self.n, nat.ILLEGAL_NOOP, 1, self.stream), "gbl_step_into")

    def check_equal(self):
        """(a) and (b) play the same games: every array they share, and the value from (b)'s wins and losses."""
        self.restore(); self.fused(); torch.cuda.synchronize()
        end_a = (self.st.clone(), self.tm.clone(), self.dn.clone())
        self.restore(); self.composed(); torch.cuda.synchronize()
        n = self.n
        for k in ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation", "nodes"):
            assert torch.equal(self.a[k][:, :n], self.b[k][:, :n]), k
        assert torch.equal(self.a["visits"][:, :n].to(torch.int32), self.b["visits"][:, :n])
        assert torch.equal(self.a["value"][:, :n], (self.b["wins"] - self.b["losses"])[:, :n].sum(2, dtype=torch.int32))
        assert all(torch.equal(x, y) for x, y in zip(end_a, (self.st, self.tm, self.dn)))

    def time(self, reps=REPS):
        """[ms of (a)], [ms of (b)]: alternating, after a warm-up of each."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = {"fused": [], "composed": []}
        for rep in range(reps + 1):
            for name in ("fused", "composed"):
                self.restore()
                torch.cuda.synchronize()
                e0.record()
                getattr(self, name)()
                e1.record()
                torch.cuda.synchronize()
                if rep:  # (repetition 0 is the warm-up)
                    out[name].append(e0.elapsed_time(e1))
        return out["fused"], out["composed"]


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def within_spread(a, b):
    return stats(a)["median"] <= stats(b)["median"] + (max(b) - min(b))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--trace":
        n, I, P = (int(x) for x in args[1:4])
        r = Runner(*states(n), I, P)
        for _ in range(3):
            r.restore(); r.fused()
        torch.cuda.synchronize()
        return
    out_path = args[0] if args else DEFAULT_OUT
    r08 = os.path.join(ROOT, "profiles", "r08", "tree_policy.json")
    per_decision = {(r["boards"], r["iterations"], r["playouts"]): r["ms_per_launch"] for r in json.load(open(r08))["rows"]} \
        if os.path.exists(r08) else {}
    rows, cache = [], {}
    for n, I, P in POINTS:
        if n not in cache:
            cache = {n: states(n)}
        r = Runner(*cache[n], I, P)
        r.check_equal()
        a, b = r.time()
        row = {"boards": n, "iterations": I, "playouts": P, "plies": T, "max_plies": M, "explore": X, "fused_ms": stats(a),
               "composed_ms": stats(b), "ratio": stats(a)["median"] / stats(b)["median"], "within_spread": within_spread(a, b),
               "fused_ms_per_ply": stats(a)["median"] / T, "tree_search_ms_per_decision_r08": per_decision.get((n, I, P))}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0),
           "method": "HIP events around one gbl_collect_search launch (fused) / the loop of gbl_tree_search + gbl_step_into (composed); "
                     "tree against tree from the same C5 position and ply index, state restored outside the timed region; one warm-up "
                     "each, then %d repetitions alternating fused and composed; ms per %d plies" % (REPS, T),
           "rows": rows}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
