#!/usr/bin/env python3
"""gbl_collect_search_tb (tablebase play and per-ply verdicts inside the self-play launch) on the complete (2, 2, 2) table, from the
stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE config 5), T = 16 plies.

    python scripts/bench_selfplay_tb.py play [out.json]      table against table and table against random, fused against composed
    python scripts/bench_selfplay_tb.py judge [out.json]     the judge beside an evaluator window, against gbl_collect_search_solve
    python scripts/bench_selfplay_tb.py census [out.json]    Tablebase.judge on a 4 096-board window of evaluator self-play
    python scripts/bench_selfplay_tb.py meta [out.json]      k_collect_tb's registers, LDS and scratch from the built library (no GPU)

(default out: profiles/r24/selfplay_tb.json; every section merges into it.  One section per process, each under its own time limit.)

  play    (a) fused: ONE gbl_collect_search_tb launch of T plies, all three judge arrays written;
          (b) composed: per ply gbl_tb_probe, the pick (torch: the probe's action where the table side moves and has one, else
              gbl_sample's draw of the ply), gbl_step_into into slot t of the trajectory arrays.
          Both start every repetition from the same position and play the same games: check_equal compares (b)'s trajectory with (a)'s
          -- the actions, every step output and the three judge arrays against the probe's outputs -- before anything is timed.
  judge   evaluator against evaluator (seeded integer network, H 64, 64 iterations, explore 16), guard depth 0 and 3: ONE
          gbl_collect_search_tb launch with the three judge arrays against ONE gbl_collect_search_solve launch on the same boards.
Method: HIP events, one warm-up each, then REPS repetitions alternating; median, min and max."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
from bench_selfplay_search import REPS, T, stats, states, within_spread  # noqa: E402,F401
from bench_solver import merge  # noqa: E402

DEV = "cuda:0"
X, I, H = 16, 64, 64
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r24", "selfplay_tb.json")
PLY0 = 100
STEP = ("actions", "winner", "rewards", "done", "to_move", "action_mask", "observation")


def full_table(inventory=(2, 2, 2)):
    tb = G.Tablebase(inventory, DEV)
    tb.build(slice_positions=1 << 28)
    assert tb.complete
    return tb


class Runner:
    """One position, two ways to play `plies` plies of the table against `other` ("tablebase" or "random") from it."""

    def __init__(self, st0, tm0, tb, other="tablebase", plies=T, seed=0, mode=0, count=1):
        self.n, self.T, self.seed, self.tb, self.mode, self.count = st0.shape[0], plies, seed, tb, mode, count
        self.policies = (nat.POLICY_TABLEBASE, nat.POLICY_TABLEBASE if other == "tablebase" else nat.POLICY_RANDOM)
        self.st0, self.tm0 = st0, tm0
        n, dev = self.n, st0.device
        self.slot = -(-n // 128) * 128
        self.st, self.tm, self.dn = st0.clone(), tm0.clone(), torch.zeros(n, dtype=torch.int8, device=dev)
        z = lambda dt, *tail: torch.zeros((plies, self.slot) + tail, dtype=dt, device=dev)  # noqa: E731

        def arrays():
            return dict(actions=z(torch.int32), winner=z(torch.int8), rewards=z(torch.int8, 2), done=z(torch.int8), to_move=z(torch.int8),
                        action_mask=z(torch.int8, 54), observation=z(torch.int8, 117), visits=z(torch.int16, 54), nodes=z(torch.int32),
                        value=z(torch.int32), how=z(torch.int8), mover=z(torch.int8), tb_outcomes=z(torch.int8, 54), tb_value=z(torch.int8),
                        tb_played=z(torch.int8))
        self.a, self.b = arrays(), arrays()
        self.b.update(act=torch.zeros(n, dtype=torch.int32, device=dev), star=torch.zeros(n, dtype=torch.int32, device=dev),
                      drawn=torch.zeros(n, dtype=torch.int32, device=dev), mask0=torch.zeros((n, 54), dtype=torch.int8, device=dev))
        self.stream = nat.current_stream(dev)
        nat.check(nat.lib().gbl_legal_mask(nat.ptr(st0), nat.ptr(tm0), nat.ptr(self.b["mask0"]), n, self.stream), "gbl_legal_mask")

    def restore(self):
        self.st.copy_(self.st0); self.tm.copy_(self.tm0); self.dn.zero_()

    def fused(self):
        a, p, tb = self.a, nat.ptr, self.tb
        nat.check(nat.lib().gbl_collect_search_tb(
            p(self.st), p(self.tm), p(self.dn), p(a["actions"]), p(a["winner"]), p(a["rewards"]), p(a["done"]), p(a["to_move"]),
            p(a["action_mask"]), p(a["observation"]), p(a["visits"]), p(a["value"]), p(a["nodes"]), p(a["how"]), p(a["mover"]), None, None,
            None, None, self.n, self.slot, 64, self.seed, 0, PLY0, None, self.T, *self.policies, None, None, 0, 0, 0, 0, 0, 0, X, 0,
            nat.ILLEGAL_NOOP, None, None, tb._inv, p(tb._aux), p(tb.table), self.mode, self.count, p(a["tb_outcomes"]), p(a["tb_value"]),
            p(a["tb_played"]), self.stream), "gbl_collect_search_tb")

    def composed(self):
        b, p, L, n, tb = self.b, nat.ptr, nat.lib(), self.n, self.tb
        for t in range(self.T):
            out, V = b["tb_outcomes"][t][:n], b["tb_value"][t][:n]
            nat.check(L.gbl_tb_probe(tb._inv, p(tb._aux), p(tb.table), p(self.st), p(self.tm), None, p(out), p(V), p(b["star"]), n,
                                     self.stream), "gbl_tb_probe")
            mask = b["mask0"] if t == 0 else b["action_mask"][t - 1][:n]
            nat.check(L.gbl_sample(p(mask), p(b["drawn"]), n, self.seed, 0, PLY0 + t, self.stream), "gbl_sample")
            table_moves = (b["star"] >= 0) if self.policies[1] == nat.POLICY_TABLEBASE else (b["star"] >= 0) & (self.tm == 0)
            torch.where(table_moves, b["star"], b["drawn"], out=b["act"])  # the pick
            b["tb_played"][t][:n] = torch.where(b["act"] >= 0, out.gather(1, b["act"].clamp(min=0).long()[:, None])[:, 0],
                                                torch.full_like(V, nat.SOLVE_NONE))
            nat.check(L.gbl_step_into(p(self.st), p(self.tm), p(self.dn), p(b["act"]), p(b["winner"][t]), p(b["rewards"][t]),
                                      p(b["action_mask"][t]), p(b["observation"][t]), None, p(b["actions"][t]), p(b["done"][t]),
                                      p(b["to_move"][t]), n, nat.ILLEGAL_NOOP, 1, self.stream), "gbl_step_into")

    def check_equal(self):
        """(a) and (b) play the same games: the step outputs and the judge arrays (the probe's outputs); both end on the same boards."""
        self.restore(); self.fused(); torch.cuda.synchronize()
        end_a = (self.st.clone(), self.tm.clone(), self.dn.clone())
        self.restore(); self.composed(); torch.cuda.synchronize()
        n = self.n
        for k in STEP + ("tb_outcomes", "tb_value", "tb_played"):
            assert torch.equal(self.a[k][:, :n], self.b[k][:, :n]), k
        assert all(torch.equal(x, y) for x, y in zip(end_a, (self.st, self.tm, self.dn)))

    def time(self, reps=REPS, names=("fused", "composed")):
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


def play(path):
    tb = full_table()
    rows = []
    for n in (4096, 65536):
        st, tm = states(n)
        for other in ("tablebase", "random"):
            r = Runner(st, tm, tb, other)
            r.check_equal()
            t = r.time()
            how = r.a["how"][:, :n]
            row = {"boards": n, "plies": T, "policies": ["tablebase", other], "fused_ms": stats(t["fused"]), "composed_ms": stats(t["composed"]),
                   "fused_over_composed": stats(t["fused"])["median"] / stats(t["composed"])["median"],
                   "within_spread": within_spread(t["fused"], t["composed"]), "table_plies": float((how == nat.HOW_TABLE).float().mean())}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del r
            torch.cuda.empty_cache()
            merge(path, "play", rows)
    merge(path, "device", torch.cuda.get_device_name(0))
    merge(path, "method", "HIP events; the complete (2, 2, 2) table; both sides from the same masked-random position, state restored outside "
          "the timed region; check_equal first; one warm-up each, then %d repetitions alternating; ms per %d plies" % (REPS, T))


def judge(path):
    from bench_selfplay_eval import seeded_evaluator
    from bench_selfplay_solve import Runner as SolveRunner
    tb = full_table()
    rows = []
    ev = seeded_evaluator(H)
    for n, depth in ((4096, 0), (4096, 3), (65536, 0), (65536, 3)):
        st, tm = states(n)
        r = SolveRunner(st, tm, I, ev, depth)
        a, p = r.a, nat.ptr
        judge_arrays = [torch.zeros((T, r.slot) + tail, dtype=torch.int8, device=DEV) for tail in ((54,), (), ())]

        def judged():
            e = C.addressof(r.struct)
            nat.check(nat.lib().gbl_collect_search_tb(
                *r._head(a), p(a["outcomes"]), p(a["proven"]), r.n, r.slot, 64, r.seed, 0, 100, None, r.T, nat.POLICY_EVAL_TREE,
                nat.POLICY_EVAL_TREE, e, e, I, I, depth, depth, 0, 0, X, 0, nat.ILLEGAL_NOOP, None, None, tb._inv, p(tb._aux), p(tb.table), 0, 1,
                *[p(x) for x in judge_arrays], r.stream), "gbl_collect_search_tb")
        r.judged = judged
        t = r.time(names=("fused", "judged"))
        row = {"boards": n, "plies": T, "iterations": I, "hidden": H, "solve_depth": depth, "gbl_collect_search_solve_ms": stats(t["fused"]),
               "gbl_collect_search_tb_judge_ms": stats(t["judged"]),
               "judge_over_plain": stats(t["judged"])["median"] / stats(t["fused"])["median"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
        merge(path, "judge_overhead", rows)
        del r
        torch.cuda.empty_cache()


def census(path):
    from bench_selfplay_eval import seeded_evaluator
    tb = full_table()
    n = 4096
    st, tm = states(n)
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=11, track_turn=True)
    env.squares.copy_(st); env.to_move.copy_(tm)
    traj = env.collect(1, policies=("evaluator", "evaluator"), refresh=False,
                       search=dict(evaluator=seeded_evaluator(H), iterations=I, explore=X, tablebase=tb, judge=True))
    counts = tb.judge(traj)
    v = traj["tb_value"][0]
    merge(path, "census_from_one_launch", {
        "boards": n, "positions": "masked-random mix (seed 11, 64 plies)", "network": "seeded int8 weights, H %d (untrained)" % H,
        "iterations": I, "won_boards": int((v > 0).sum()), "drawn_boards": int(((v == 0) & (traj["z_exact"][0] != nat.Z_OPEN)).sum()),
        "lost_boards": int((v < 0).sum()), "regret": counts})
    print(counts, flush=True)


def meta(path):
    import subprocess
    from tests.test_abi_and_host import kernel_metadata
    md = {k: v for k, v in kernel_metadata(None).items() if "k_collect_tb" in k}
    names = subprocess.run(["c++filt"] + list(md), capture_output=True, text=True).stdout.splitlines()
    out = {}
    for name, v in zip(names, md.values()):
        name = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        out[name] = {"vgpr": int(v["vgpr_count"]), "sgpr": int(v["sgpr_count"]), "lds": int(v["group_segment_fixed_size"]),
                     "scratch": int(v["private_segment_fixed_size"]), "vgpr_spill": int(v["vgpr_spill_count"])}
    merge(path, "kernel_resources", {"template": "k_collect_tb<NOISE, SEARCH>", "kernels": out})
    print(out)


def main():
    args = sys.argv[1:]
    what = args[0] if args else "play"
    path = args[1] if len(args) > 1 else DEFAULT_OUT
    {"play": play, "judge": judge, "census": census, "meta": meta}[what](path)


if __name__ == "__main__":
    main()
