#!/usr/bin/env python3
"""The Gumbel root search (gbl_tree_search_gumbel, gbl_collect_search_gumbel): what the root rule costs beside the PUCT search, what a
small-budget Gumbel window costs and keeps beside the windows it is meant to replace, and how it plays.  Shapes as
scripts/bench_selfplay_cap.py: the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), BASELINE config 5), one seeded
integer network (H 64), explore 16.

    python scripts/bench_gumbel.py [out.json] [--parent lib.so]    on the GPU (default out: profiles/r29/gumbel.json)
    python scripts/bench_gumbel.py [out.json] --host [--games 128]  the strength tables, on the host flavour (bit-identical to the device)

Device, at 4 096 and 65 536 boards, HIP events, one warm-up each, then 5 repetitions alternating in one process, median with minimum and
maximum, the state restored outside the timed region:
  search   gbl_tree_search_gumbel (considered 16, noise on, 50 / 23) against gbl_tree_search_eval at 16 and at 64 iterations, and
           gbl_tree_search_eval of this build against a library built from the PARENT commit (--parent: scripts/build_variant.sh makes it
           from a checkout of that commit; without it the comparison is recorded as NOT MEASURED): the same instantiation, so it must lie
           inside the parent's own min-max spread;
  window   16 plies of evaluator against evaluator: gbl_collect_search_gumbel at 16 iterations (considered 16 on both sides) against the
           parent build's gbl_collect_search_eval at 64 iterations (this build's without --parent) and against gbl_collect_search_cap
           (64 iterations, 16 on a fast ply, share 1/4, noise weight 64), with the kept rows per second of each.  Kept rows: the cells
           whose visits row is not zero (what gbl_training_batch and gbl_replay_append can keep).
Host: the example's network (examples/example_train_evaluator.py, as DESIGN 5.10 used it), `games` games per pairing, half as each colour,
Gumbel(16) against PUCT(16) and PUCT(64), and a sweep of scale {8, 23, 46} x considered {4, 16} against PUCT(16).  One short training
run, one seed: no claim beyond the table."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
from bench_selfplay_eval import seeded_evaluator  # noqa: E402
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402
from bench_selfplay_solve import PLY0, Runner, H, X  # noqa: E402
from bench_solver import merge  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r29", "gumbel.json")
BOARDS = (4096, 65536)
CONSIDERED, OFFSET, SCALE = 16, 50, 23
SMALL, LARGE = 16, 64  # the Gumbel window's budget, and the PUCT window's
NOISE, SHARE = 64, 64  # the capped window's noise weight and its share of full plies (1/4)


def load_parent(path):
    L = C.CDLL(os.path.abspath(path))
    for name in ("gbl_tree_search_eval", "gbl_collect_search_eval", "gbl_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L


class SearchRunner:
    """One batch of positions and one set of outputs; a decision by the PUCT search of this build, of a parent build, and by the Gumbel
    search."""

    def __init__(self, st, tm, iterations, ev, parent=None):
        n, dev = st.shape[0], st.device
        self.n, self.I, self.st, self.tm, self.parent_lib = n, iterations, st, tm, parent
        z = lambda dt, *tail: torch.zeros((n,) + tail, dtype=dt, device=dev)  # noqa: E731
        self.out = [z(torch.int32, 54), z(torch.int32, 54), z(torch.int32, 54), z(torch.int32), z(torch.int32), z(torch.int32), z(torch.uint8, 54)]
        self.target, self.g = z(torch.uint8, 54), z(torch.int16, 54)
        self.struct, self.stream = ev.as_struct(), nat.current_stream(dev)

    def _eval(self, lib, name):
        nat.check(lib.gbl_tree_search_eval(self.st.data_ptr(), self.tm.data_ptr(), None, C.addressof(self.struct), self.I, X,
                                           *[o.data_ptr() for o in self.out], self.n, self.stream), name)

    def eval(self):
        self._eval(nat.lib(), "gbl_tree_search_eval")

    def parent(self):
        self._eval(self.parent_lib, "gbl_tree_search_eval (parent)")

    def gumbel(self):
        nat.check(nat.lib().gbl_tree_search_gumbel(self.st.data_ptr(), self.tm.data_ptr(), None, C.addressof(self.struct), self.I, X, CONSIDERED,
                                                   1, OFFSET, SCALE, 0, 0, 7, *[o.data_ptr() for o in self.out], self.target.data_ptr(),
                                                   self.g.data_ptr(), self.n, self.stream), "gbl_tree_search_gumbel")

    def time(self, reps=REPS, names=("eval", "gumbel")):
        """{name: [ms]}: alternating, after a warm-up of each."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = {k: [] for k in names}
        for rep in range(reps + 1):
            for name in names:
                torch.cuda.synchronize()
                e0.record()
                getattr(self, name)()
                e1.record()
                torch.cuda.synchronize()
                if rep:  # (repetition 0 is the warm-up)
                    out[name].append(e0.elapsed_time(e1))
        return out


class WindowRunner(Runner):
    """bench_selfplay_solve's position and arrays; the three windows."""

    def __init__(self, *args, parent=None, **kw):
        super().__init__(*args, **kw)
        self.parent_lib = parent

    def _tail(self, iterations):
        e = C.addressof(self.struct)
        return (self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T, nat.POLICY_EVAL_TREE, nat.POLICY_EVAL_TREE, e, e, iterations, iterations)

    def gumbel(self):
        nat.check(nat.lib().gbl_collect_search_gumbel(*self._head(self.a), *self._tail(SMALL), X, 0, nat.ILLEGAL_NOOP, None, None, CONSIDERED,
                                                      CONSIDERED, 1, OFFSET, SCALE, self.stream), "gbl_collect_search_gumbel")

    def puct(self):
        lib = self.parent_lib if self.parent_lib is not None else nat.lib()
        nat.check(lib.gbl_collect_search_eval(*self._head(self.b), *self._tail(LARGE), X, 0, nat.ILLEGAL_NOOP, None, None, self.stream),
                  "gbl_collect_search_eval")

    def cap(self):
        c = self.c
        nat.check(nat.lib().gbl_collect_search_cap(*self._head(c), nat.ptr(c["outcomes"]), nat.ptr(c["proven"]), *self._tail(LARGE), 0, 0, NOISE,
                                                   NOISE, X, 0, nat.ILLEGAL_NOOP, None, None, SMALL, SMALL, SHARE, SHARE, self.stream),
                  "gbl_collect_search_cap")

    def census(self, arrays):
        n = self.n
        return {"kept_rows": int((arrays["visits"][:, :n].to(torch.int32).sum(-1) > 0).sum()),
                "evaluations": int(arrays["nodes"][:, :n].to(torch.int64).sum())}


def device(path, parent_path):
    parent = load_parent(parent_path) if parent_path else None
    ev = seeded_evaluator(H)
    search_rows, window_rows = [], []
    for n in BOARDS:
        st, tm = states(n)
        for its in (SMALL, LARGE):
            r = SearchRunner(st, tm, its, ev, parent)
            t = r.time(names=("eval", "gumbel") + (("parent",) if parent is not None else ()))
            e, g = stats(t["eval"]), stats(t["gumbel"])
            row = {"boards": n, "iterations": its, "hidden": H, "explore": X, "considered": CONSIDERED, "visit_offset": OFFSET, "scale": SCALE,
                   "eval_ms": e, "gumbel_ms": g, "gumbel_over_eval": g["median"] / e["median"]}
            if parent is not None:
                p = stats(t["parent"])
                row.update(parent_eval_ms=p, parent_spread_ms=p["max"] - p["min"], eval_over_parent=e["median"] / p["median"],
                           eval_within_parent_spread=within_spread(t["eval"], t["parent"]))
            else:
                row.update(parent_eval_ms="NOT MEASURED")
            print(json.dumps(row), flush=True)
            search_rows.append(row)
            del r
        w = WindowRunner(st, tm, LARGE, ev, 0, parent=parent)
        t = w.time(reps=REPS, names=("puct", "gumbel", "cap"))
        row = {"boards": n, "plies": T, "hidden": H, "explore": X, "puct_is": "parent build" if parent is not None else "this build (parent NOT MEASURED)"}
        base = stats(t["puct"])["median"]
        for name, arrays, what in (("puct", w.b, "gbl_collect_search_eval, %d iterations" % LARGE),
                                   ("gumbel", w.a, "gbl_collect_search_gumbel, %d iterations, considered %d" % (SMALL, CONSIDERED)),
                                   ("cap", w.c, "gbl_collect_search_cap, %d iterations, %d on a fast ply, share %d / 256, noise %d" % (LARGE, SMALL, SHARE, NOISE))):
            w.restore(); getattr(w, name)(); torch.cuda.synchronize()
            c, s = w.census(arrays), stats(t[name])
            row[name] = {"what": what, "ms": s, "over_puct": s["median"] / base, "census": c, "kept_rows_per_s": c["kept_rows"] / (s["median"] * 1e-3),
                         "evaluations_per_kept_row": c["evaluations"] / max(c["kept_rows"], 1)}
        print(json.dumps(row), flush=True)
        window_rows.append(row)
        del w
        torch.cuda.empty_cache()
        merge(path, "search", search_rows)
        merge(path, "window", window_rows)
    merge(path, "device", torch.cuda.get_device_name(0))
    merge(path, "method", "HIP events; one seeded int8 network (H %d), explore %d, C5 positions; one warm-up each, then %d repetitions alternating in "
          "one process; search: ms per decision batch; window: ms per %d plies of evaluator against evaluator from the same position, the state "
          "restored outside the timed region; parent = a library built from the parent commit; kept rows = cells with a non-zero visits row"
          % (H, X, REPS, T))
    print("wrote", path)


def host(path, games):
    import example_train_evaluator as EX
    nat.cpu_raw().gbl_cpu_set_threads(0)
    ev, samples, loss = EX.train_evaluator("cpu")

    def play(gumbel, iterations, other_iterations):
        """Gumbel(iterations) against PUCT(other_iterations), half as each colour: (wins, losses, unfinished) of the Gumbel search."""
        mine = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=iterations, gumbel=gumbel, seed=5, device="cpu")
        theirs = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=other_iterations, device="cpu")
        w1, l1 = EX.arena(mine, theirs, games // 2, "cpu")
        l2, w2 = EX.arena(theirs, mine, games // 2, "cpu")
        return {"wins": w1 + w2, "losses": l1 + l2, "unfinished": 2 * (games // 2) - w1 - w2 - l1 - l2}
    default = dict(considered=CONSIDERED, visit_offset=OFFSET, scale=SCALE)
    rec = {"trained_evaluator": {"samples": samples, "final_loss": loss, "hidden": ev.hidden}, "games": 2 * (games // 2), "gumbel": default,
           "note": "PUCT is deterministic: against it every game differs only through the Gumbel side's noise (seed 5, the board id)",
           "gumbel16_vs_puct16": play(default, SMALL, SMALL), "gumbel16_vs_puct64": play(default, SMALL, LARGE), "sweep_vs_puct16": []}
    print(json.dumps(rec), flush=True)
    for scale in (8, 23, 46):
        for considered in (4, 16):
            row = dict(scale=scale, considered=considered, **play(dict(default, scale=scale, considered=considered), SMALL, SMALL))
            print(json.dumps(row), flush=True)
            rec["sweep_vs_puct16"].append(row)
    merge(path, "strength_host_flavour", rec)
    print("wrote", path)


def main():
    args = sys.argv[1:]
    parent, games, on_host = None, 128, "--host" in args
    if on_host:
        args.remove("--host")
    for flag in ("--parent", "--games"):
        if flag in args:
            i = args.index(flag)
            if flag == "--parent":
                parent = args[i + 1]
            else:
                games = int(args[i + 1])
            del args[i:i + 2]
    path = args[0] if args else DEFAULT_OUT
    if on_host:
        host(path, games)
    else:
        device(path, parent)


if __name__ == "__main__":
    main()
