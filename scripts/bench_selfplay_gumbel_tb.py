#!/usr/bin/env python3
"""gbl_collect_gumbel_tb (the tablebase and its judge in the Gumbel self-play window): in one process, on the stationary masked-random
mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE config 5) and the complete (2, 2, 2) table, one seeded integer network (H 64),
Gumbel with 16 iterations and 16 considered actions, explore 16, T = 16.

    python scripts/bench_selfplay_gumbel_tb.py [out.json] [--parent lib.so]   on the GPU (default out: profiles/r33/selfplay_gumbel_tb.json)
    python scripts/bench_selfplay_gumbel_tb.py --host [out.json]              the census on the host flavour (no GPU)

Per point (boards 4 096 / 65 536), alternating, median of five with min - max:
  fused      ONE gbl_collect_gumbel_tb launch of T plies, a Gumbel-16 side (player_1) against the table (player_2), the three judge arrays
             written;
  composed   per ply: gbl_tb_probe of the whole batch; gbl_tree_search_gumbel(call = the ply index) on the WHOLE batch under the legal
             mask on the boards the Gumbel side moves and an empty row on the others (the Gumbel row's board id is env_base + the row, so
             the sub-batch cannot be gathered); gbl_sample for the boards the table does not hold; a torch pick between the three;
             tb_played by a gather; gbl_step_into into slot t.  It plays the same games: its trajectory is compared with the fused one's
             before anything is timed (the table ply's visits row is the fused launch's own: the loop does not restate it);
  judged     ONE gbl_collect_gumbel_tb launch, Gumbel-16 against Gumbel-16 with the three judge arrays (k_collect_gumbel_tb);
  gumbel     ONE gbl_collect_search_gumbel launch on the same boards (k_collect_eval<true>), of this build and (--parent) of a library
             built from the parent commit: what the judge costs a Gumbel window is judged / parent's gumbel;
  posthoc    `gumbel`, then gbl_decode_obs + gbl_tb_probe over all T x N stored cells: the judge a user has without this entry point;
  tb         ONE gbl_collect_search_tb launch, table against table with the judge, of this build and (--parent) the parent's.
This build's `gumbel` and `tb` are held against the parent's min - max band.  `guard`: 4 096 boards x 16 plies, fused against composed
-- the row tests/test_gpu_gumbel_tb_guard.py measures again.

--host: on the host flavour (bit-identical to the kernels) and the complete (2, 2, 0) table, one 16-ply window each of Gumbel-16 and
of PUCT-64 self-play from the same start boards, every ply judged: won / drawn / lost positions, plies that keep the result and regret
1 / 2 / 3 per side.  One seed: no claim beyond the table."""
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
from bench_gumbel import CONSIDERED, LARGE, OFFSET, SCALE, SMALL, WindowRunner  # noqa: E402
from bench_selfplay_eval import seeded_evaluator  # noqa: E402
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402,F401
from bench_selfplay_solve import PLY0, H, X  # noqa: E402
from bench_selfplay_tb import full_table  # noqa: E402,F401
from bench_solver import merge  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r33", "selfplay_gumbel_tb.json")
BOARDS = (4096, 65536)
SHARED = ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation", "nodes", "root_value", "priors", "tb_outcomes",
          "tb_value", "tb_played")
EVAL, TABLE = nat.POLICY_EVAL_TREE, nat.POLICY_TABLEBASE


def load_parent(path):
    L = C.CDLL(os.path.abspath(path))
    for name in ("gbl_collect_search_gumbel", "gbl_collect_search_tb", "gbl_last_error"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    return L


class TableRunner(WindowRunner):
    """bench_selfplay_solve's position and arrays (a: fused / judged, b: composed, c: the unjudged windows) and the judge's three beside
    each."""

    def __init__(self, st0, tm0, ev, tb, plies=T, parent=None, mode=0, count=1):
        super().__init__(st0, tm0, SMALL, ev, 0, plies=plies, parent=parent)
        n, dev = self.n, st0.device
        self.tb, self.mode, self.count = tb, mode, count
        z = lambda dt, *tail: torch.zeros((n,) + tail, dtype=dt, device=dev)  # noqa: E731
        for arrays in (self.a, self.b, self.c):
            arrays.update(tb_outcomes=torch.zeros((plies, self.slot, 54), dtype=torch.int8, device=dev),
                          tb_value=torch.zeros((plies, self.slot), dtype=torch.int8, device=dev),
                          tb_played=torch.zeros((plies, self.slot), dtype=torch.int8, device=dev))
        self.tree = [z(torch.int32, 54), z(torch.int32, 54), z(torch.int32, 54), z(torch.int32), z(torch.int32), z(torch.int32), z(torch.uint8, 54)]
        self.target, self.mask, self.mask0 = z(torch.uint8, 54), z(torch.int8, 54), z(torch.int8, 54)
        self.star, self.drawn = z(torch.int32), z(torch.int32)
        cells = plies * self.slot  # (the post-hoc judge's scratch: a board, a mover and a verdict per stored cell)
        self.cell_state, self.cell_tm = torch.zeros((cells, 27), dtype=torch.int8, device=dev), torch.zeros(cells, dtype=torch.int8, device=dev)
        self.cell_out, self.cell_v = torch.zeros((cells, 54), dtype=torch.int8, device=dev), torch.zeros(cells, dtype=torch.int8, device=dev)
        nat.check(nat.lib().gbl_legal_mask(nat.ptr(st0), nat.ptr(tm0), nat.ptr(self.mask0), n, self.stream), "gbl_legal_mask")

    def _window(self, p0, p1, iterations):
        e = C.addressof(self.struct)
        return (self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T, p0, p1, e if p0 == EVAL else None, e if p1 == EVAL else None,
                iterations if p0 == EVAL else 0, iterations if p1 == EVAL else 0)

    def _rule(self):
        return (X, 0, nat.ILLEGAL_NOOP, None, None, CONSIDERED, CONSIDERED, 1, OFFSET, SCALE)

    def _table(self, a):
        tb, p = self.tb, nat.ptr
        return (tb._inv, p(tb._aux), p(tb.table), self.mode, self.count, p(a["tb_outcomes"]), p(a["tb_value"]), p(a["tb_played"]))

    def fused(self):
        nat.check(nat.lib().gbl_collect_gumbel_tb(*self._head(self.a), *self._window(EVAL, TABLE, SMALL), *self._rule(), *self._table(self.a),
                                                  self.stream), "gbl_collect_gumbel_tb")

    def judged(self):
        nat.check(nat.lib().gbl_collect_gumbel_tb(*self._head(self.a), *self._window(EVAL, EVAL, SMALL), *self._rule(), *self._table(self.a),
                                                  self.stream), "gbl_collect_gumbel_tb")

    def composed(self):
        b, p, L, e, n, tb = self.b, nat.ptr, nat.lib(), C.addressof(self.struct), self.n, self.tb
        vis_, w_, l_, act_, nd_, rv_, pr_ = self.tree
        for t in range(self.T):
            out, V = b["tb_outcomes"][t][:n], b["tb_value"][t][:n]
            nat.check(L.gbl_tb_probe(tb._inv, p(tb._aux), p(tb.table), p(self.st), p(self.tm), None, p(out), p(V), p(self.star), n, self.stream),
                      "gbl_tb_probe")
            legal = self.mask0 if t == 0 else b["action_mask"][t - 1][:n]
            rule = self.tm == 0  # the boards the Gumbel side moves
            torch.mul(legal, rule[:, None], out=self.mask)
            nat.check(L.gbl_tree_search_gumbel(p(self.st), p(self.tm), p(self.mask), e, SMALL, X, CONSIDERED, 1, OFFSET, SCALE, self.seed, 0,
                                               PLY0 + t, p(vis_), p(w_), p(l_), p(act_), p(nd_), p(rv_), p(pr_), p(self.target), None, n,
                                               self.stream), "gbl_tree_search_gumbel")
            nat.check(L.gbl_sample(p(legal), p(self.drawn), n, self.seed, 0, PLY0 + t, self.stream), "gbl_sample")
            # the pick: the rule's action, the table's where it has one, the masked-random draw elsewhere
            torch.where(rule, act_, torch.where(self.star >= 0, self.star, self.drawn), out=act_)
            b["visits"][t][:n] = torch.where(rule[:, None], self.target.to(torch.int16), 0)
            b["nodes"][t][:n] = torch.where(rule, nd_, 0)
            b["root_value"][t][:n] = torch.where(rule, rv_, 0)
            b["priors"][t][:n] = torch.where(rule[:, None], pr_, 0)
            b["tb_played"][t][:n] = torch.where(act_ >= 0, out.gather(1, act_.clamp(min=0).long()[:, None])[:, 0],
                                                torch.full_like(V, nat.SOLVE_NONE))
            nat.check(L.gbl_step_into(p(self.st), p(self.tm), p(self.dn), p(act_), p(b["winner"][t]), p(b["rewards"][t]),
                                      p(b["action_mask"][t]), p(b["observation"][t]), None, p(b["actions"][t]), p(b["done"][t]),
                                      p(b["to_move"][t]), n, nat.ILLEGAL_NOOP, 1, self.stream), "gbl_step_into")

    def gumbel(self, lib=None):
        nat.check((lib or nat.lib()).gbl_collect_search_gumbel(*self._head(self.c), *self._window(EVAL, EVAL, SMALL), *self._rule(), self.stream),
                  "gbl_collect_search_gumbel")

    def parent_gumbel(self):
        self.gumbel(self.parent_lib)

    def posthoc(self):
        c, p, L, tb = self.c, nat.ptr, nat.lib(), self.tb
        self.gumbel()
        cells = self.T * self.slot
        nat.check(L.gbl_decode_obs(p(c["observation"]), p(self.cell_state), p(self.cell_tm), cells, self.stream), "gbl_decode_obs")
        nat.check(L.gbl_tb_probe(tb._inv, p(tb._aux), p(tb.table), p(self.cell_state), p(self.cell_tm), None, p(self.cell_out), p(self.cell_v),
                                 None, cells, self.stream), "gbl_tb_probe")

    def tb_window(self, lib=None):
        c = self.c
        nat.check((lib or nat.lib()).gbl_collect_search_tb(*self._head(c), None, None, *self._window(TABLE, TABLE, 0), 0, 0, 0, 0, X, 0,
                                                           nat.ILLEGAL_NOOP, None, None, *self._table(c), self.stream), "gbl_collect_search_tb")

    def parent_tb_window(self):
        self.tb_window(self.parent_lib)

    def check_equal(self):
        """fused and composed play the same games: every array they share, the Gumbel plies' target rows, and the boards they end on."""
        self.restore(); self.fused(); torch.cuda.synchronize()
        end_a = (self.st.clone(), self.tm.clone(), self.dn.clone())
        self.restore(); self.composed(); torch.cuda.synchronize()
        n = self.n
        for k in SHARED:
            assert torch.equal(self.a[k][:, :n], self.b[k][:, :n]), k
        rule = self.a["how"][:, :n] == nat.HOW_GUMBEL
        assert rule.any() and torch.equal(self.a["visits"][:, :n][rule], self.b["visits"][:, :n][rule])
        assert not self.b["visits"][:, :n][~rule].any()
        assert all(torch.equal(x, y) for x, y in zip(end_a, (self.st, self.tm, self.dn)))


def census_of(tb, traj, boards=None):
    """Tablebase.judge's counts with the positions' values beside them, per side."""
    counts = tb.judge(traj, boards)
    v, z, mover = traj["tb_value"], traj["z_exact"], traj["mover"]
    out = {}
    for m, name in enumerate(("player_1", "player_2")):
        mine = (mover == m) & (z != nat.Z_OPEN)
        out[name] = dict(counts[name], won_positions=int((mine & (v > 0)).sum()), drawn_positions=int((mine & (v == 0)).sum()),
                         lost_positions=int((mine & (v < 0)).sum()))
    return out


def device(path, parent_path):
    parent = load_parent(parent_path) if parent_path else None
    ev = seeded_evaluator(H)
    tb = full_table()
    rows = []
    for n in BOARDS:
        st, tm = states(n)
        r = TableRunner(st, tm, ev, tb, parent=parent)
        r.check_equal()
        # what is compared is timed together, alternating: fused / composed; the judged window, the plain one and the post-hoc judge; and
        # (--parent) each parent entry point of this build against the parent build's, in a pair of its own
        raw = {**r.time(reps=REPS, names=("fused", "composed")), **r.time(reps=REPS, names=("judged", "gumbel", "posthoc"))}
        if parent is not None:
            pair = r.time(reps=REPS, names=("gumbel", "parent_gumbel"))
            raw.update(gumbel_beside_parent=pair["gumbel"], parent_gumbel=pair["parent_gumbel"], **r.time(reps=REPS, names=("tb_window", "parent_tb_window")))
        else:
            raw.update(r.time(reps=REPS, names=("tb_window",)))
        t = {k: stats(v) for k, v in raw.items()}
        r.restore(); r.fused(); torch.cuda.synchronize()
        how = r.a["how"][:, :n]
        kept = int((r.a["visits"][:, :n].to(torch.int32).sum(-1) > 0).sum())
        row = {"boards": n, "plies": T, "hidden": H, "explore": X, "iterations": SMALL, "considered": CONSIDERED, "table": list(tb.inventory),
               "fused_ms": t["fused"], "composed_ms": t["composed"], "judged_ms": t["judged"], "gumbel_ms": t["gumbel"], "posthoc_ms": t["posthoc"],
               "tb_ms": t["tb_window"], "fused_over_composed": t["fused"]["median"] / t["composed"]["median"],
               "fused_within_composed_spread": within_spread(raw["fused"], raw["composed"]),
               "judged_over_gumbel": t["judged"]["median"] / t["gumbel"]["median"],
               "judged_over_posthoc": t["judged"]["median"] / t["posthoc"]["median"],
               "table_plies": float(((how == nat.HOW_TABLE) | (how == nat.HOW_TABLE_SAMPLED)).float().mean()),
               "gumbel_plies": float((how == nat.HOW_GUMBEL).float().mean()), "kept_rows": kept,
               "kept_rows_per_s": kept / (t["fused"]["median"] * 1e-3)}
        if parent is not None:
            row.update(parent_gumbel_ms=t["parent_gumbel"], gumbel_beside_parent_ms=t["gumbel_beside_parent"], parent_tb_ms=t["parent_tb_window"],
                       gumbel_within_parent_band=within_spread(raw["gumbel_beside_parent"], raw["parent_gumbel"]),
                       tb_within_parent_band=within_spread(raw["tb_window"], raw["parent_tb_window"]),
                       judged_over_parent_gumbel=t["judged"]["median"] / t["parent_gumbel"]["median"])
        else:
            row.update(parent_gumbel_ms="NOT MEASURED", parent_tb_ms="NOT MEASURED")
        print(json.dumps(row), flush=True)
        rows.append(row)
        if n == 4096:
            merge(path, "guard", {"boards": n, "plies": T, "fused_ms": t["fused"], "composed_ms": t["composed"],
                                  "fused_over_composed": row["fused_over_composed"], "within_spread": row["fused_within_composed_spread"]})
        del r
        torch.cuda.empty_cache()
        merge(path, "rows", rows)
    merge(path, "device", torch.cuda.get_device_name(0))
    merge(path, "method", "HIP events; the complete (2, 2, 2) table; seeded int8 weights, H %d; every window from the same C5 position, the state "
          "restored outside the timed region; check_equal first; what is compared is timed together: one warm-up each, then %d repetitions alternating in one process; ms per "
          "%d plies; parent = a library built from the parent commit; kept rows = cells with a non-zero visits row" % (H, REPS, T))
    print("wrote", path)


def host(path, boards=4096, plies=T, inventory=(2, 2, 0)):
    nat.cpu_raw().gbl_cpu_set_threads(16)
    ev = seeded_evaluator(H, "cpu")
    tb = G.Tablebase(inventory, "cpu")
    tb.build()
    assert tb.complete
    idx = torch.from_numpy(np.random.default_rng(11).integers(0, tb.positions, 2 * boards))
    idx = idx[tb.value(idx) != nat.TB_TERMINAL][:boards]  # positions nobody has won yet, player_1 to move
    assert len(idx) == boards
    start = tb.position(idx)
    recs = []
    for name, its, considered in (("Gumbel-%d" % SMALL, SMALL, CONSIDERED), ("PUCT-%d" % LARGE, LARGE, 0)):
        env = G.BatchedGobblet(boards, "cpu", auto_reset=True, seed=11, track_turn=True)
        env.squares.copy_(start)
        traj = env.collect(plies, policies=("evaluator", "evaluator"),
                           search=dict(evaluator=ev, iterations=its, explore=X,
                                       gumbel=dict(considered=considered, visit_offset=OFFSET, scale=SCALE, tablebase=tb, judge=True)))
        rec = {"side": name, "iterations": its, "considered": considered, "boards": boards, "plies": plies, "census": census_of(tb, traj)}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    merge(path, "census_host_flavour", {"network": "seeded int8 weights, H %d (untrained)" % H, "table": list(inventory),
                                        "start": "sampled positions of the table nobody has won, player_1 to move", "rows": recs,
                                        "note": "one seed, one window each from the same start boards: no claim beyond the table"})
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
