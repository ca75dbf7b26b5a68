#!/usr/bin/env python3
"""gbl_collect_search_eval (evaluator-guided self-play collection): the fused launch against the composed loop on the entry points
that existed before it, in the same process, on the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as
BASELINE config 5), evaluator against evaluator with one seeded integer network, explore 16, sample_plies 0, T = 16 plies.

    python scripts/bench_selfplay_eval.py [out.json] [--points N,I,H ...]   on the GPU (default: profiles/r12/selfplay_eval.json)

  (a) fused     ONE gbl_collect_search_eval launch of T plies;
  (b) composed  per ply: gbl_tree_search_eval into slot t of visits / wins / losses / nodes / root_value / priors arrays, then
                gbl_step_into with the search's action_out into slot t of the seven trajectory arrays -- 2 T launches and the
                action's round trip.
Both start every repetition from the same position (the state is restored outside the timed region), so they play the same games:
(b)'s trajectory is compared with (a)'s before anything is timed.  Method: HIP events around the launch / the loop, one warm-up
each, then REPS repetitions alternating (a) and (b); the record keeps median, min and max.  `within_spread` = median(a) <=
median(b) + (max(b) - min(b)), as scripts/bench_selfplay_search.py.  Every finished row is printed and the record rewritten, so an
interrupted run keeps what it measured."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402

DEV = "cuda:0"
X = 16
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r12", "selfplay_eval.json")
POINTS = tuple((n, I, H) for n in (4096, 65536) for I in (64, 256) for H in (64, 256))  # (boards, iterations, hidden)
PLY0 = 100


def seeded_evaluator(hidden, device=DEV, seed=0):
    """Ordinary random int8 weights (the cost of a search does not depend on what the network has learnt, only on its size)."""
    rng = np.random.default_rng(seed + hidden)
    return G.GobbletEvaluator(rng.integers(-128, 128, (117, hidden), dtype=np.int8), rng.integers(-300, 300, hidden),
                              rng.integers(-128, 128, (hidden // 4, 56, 4), dtype=np.int8), rng.integers(-65536, 65536, 56), 1, 9, 9,
                              device=device)


class Runner:
    """One position, two ways to play T plies of evaluator against evaluator from it into trajectory arrays of one's own."""

    def __init__(self, st0, tm0, I, ev, plies=T, seed=0):
        self.n, self.I, self.T, self.seed, self.ev = st0.shape[0], I, plies, seed, ev
        self.st0, self.tm0 = st0, tm0
        n, dev = self.n, st0.device
        self.slot = -(-n // 128) * 128
        self.st, self.tm, self.dn = st0.clone(), tm0.clone(), torch.zeros(n, dtype=torch.int8, device=dev)
        z = lambda dt, *tail: torch.zeros((plies, self.slot) + tail, dtype=dt, device=dev)  # noqa: E731

        def arrays(visit_dtype):
            return dict(actions=z(torch.int32), winner=z(torch.int8), rewards=z(torch.int8, 2), done=z(torch.int8), to_move=z(torch.int8),
                        action_mask=z(torch.int8, 54), observation=z(torch.int8, 117), visits=z(visit_dtype, 54), nodes=z(torch.int32),
                        root_value=z(torch.int32), priors=z(torch.uint8, 54))
        self.a = arrays(torch.int16)
        self.a.update(value=z(torch.int32), how=z(torch.int8), mover=z(torch.int8))
        self.b = arrays(torch.int32)
        self.b.update(wins=torch.zeros_like(self.b["visits"]), losses=torch.zeros_like(self.b["visits"]),
                      act=torch.zeros(n, dtype=torch.int32, device=dev))
        self.stream = nat.current_stream(dev)
        self.struct = ev.as_struct()

    def restore(self):
        self.st.copy_(self.st0); self.tm.copy_(self.tm0); self.dn.zero_()

    def fused(self):
        a, p, e = self.a, nat.ptr, C.addressof(self.struct)
        nat.check(nat.lib().gbl_collect_search_eval(
            p(self.st), p(self.tm), p(self.dn), p(a["actions"]), p(a["winner"]), p(a["rewards"]), p(a["done"]), p(a["to_move"]),
            p(a["action_mask"]), p(a["observation"]), p(a["visits"]), p(a["value"]), p(a["nodes"]), p(a["how"]), p(a["mover"]),
            p(a["root_value"]), p(a["priors"]), self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T, nat.POLICY_EVAL_TREE,
            nat.POLICY_EVAL_TREE, e, e, self.I, self.I, X, 0, nat.ILLEGAL_NOOP, None, None, self.stream), "gbl_collect_search_eval")

    def composed(self):
        b, p, L, e = self.b, nat.ptr, nat.lib(), C.addressof(self.struct)
        for t in range(self.T):
            nat.check(L.gbl_tree_search_eval(p(self.st), p(self.tm), None, e, self.I, X, p(b["visits"][t]), p(b["wins"][t]), p(b["losses"][t]),
                                             p(b["act"]), p(b["nodes"][t]), p(b["root_value"][t]), p(b["priors"][t]), self.n, self.stream),
                      "gbl_tree_search_eval")
            nat.check(L.gbl_step_into(p(self.st), p(self.tm), p(self.dn), p(b["act"]), p(b["winner"][t]), p(b["rewards"][t]),
                                      p(b["action_mask"][t]), p(b["observation"][t]), None, p(b["actions"][t]), p(b["done"][t]),
                                      p(b["to_move"][t]), self.n, nat.ILLEGAL_NOOP, 1, self.stream), "gbl_step_into")

    def check_equal(self):
        """(a) and (b) play the same games: every array they share, and the value from (b)'s wins and losses."""
        self.restore(); self.fused(); torch.cuda.synchronize()
        end_a = (self.st.clone(), self.tm.clone(), self.dn.clone())
        self.restore(); self.composed(); torch.cuda.synchronize()
        n = self.n
        for k in ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation", "nodes", "root_value", "priors"):
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


def main():
    args = sys.argv[1:]
    points = POINTS
    if "--points" in args:
        i = args.index("--points")
        points = tuple(tuple(int(x) for x in a.split(",")) for a in args[i + 1:])
        args = args[:i]
    out_path = args[0] if args else DEFAULT_OUT
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    rows, cache = [], {}
    for n, I, H in points:
        if n not in cache:
            cache = {n: states(n)}
        r = Runner(*cache[n], I, seeded_evaluator(H))
        r.check_equal()
        a, b = r.time()
        row = {"boards": n, "iterations": I, "hidden": H, "plies": T, "explore": X, "fused_ms": stats(a), "composed_ms": stats(b),
               "ratio": stats(a)["median"] / stats(b)["median"], "within_spread": within_spread(a, b),
               "fused_ms_per_ply": stats(a)["median"] / T}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r
        torch.cuda.empty_cache()
        rec = {"device": torch.cuda.get_device_name(0),
               "method": "HIP events around one gbl_collect_search_eval launch (fused) / the loop of gbl_tree_search_eval + gbl_step_into "
                         "(composed); evaluator against evaluator (seeded int8 weights) from the same C5 position, state restored outside the "
                         "timed region; one warm-up each, then %d repetitions alternating fused and composed; ms per %d plies" % (REPS, T),
               "rows": rows}
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
