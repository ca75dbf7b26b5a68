#!/usr/bin/env python3
"""gbl_tree_search (TreeSearchGobbletPolicy): time per launch, useful plies/s and their ratio to gbl_playout_values at the same
number of playouts per board, on the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE config 5),
plus arenas of the tree search as player_1 against depth-2 greedy and against flat Monte-Carlo at the same playouts per decision.

    python scripts/bench_tree_policy.py [out.json]         on the GPU (default: profiles/r08/tree_policy.json)
    python scripts/bench_tree_policy.py --host [out.json]  on the host flavour: the `explore` sweep and the threat study
    python scripts/bench_tree_policy.py --trace N I P      one warm launch + 3 timed ones, for rocprofv3 runs

Both modes merge their sections into the same record.  useful plies = sum of plies_out (the masked-random plies of the playouts;
gbl_playout_values' count includes its root moves, one per playout).  The host flavour is bit-identical to the kernel, so the
`explore` sweep and the threat study (tests/test_tree_policy.py: positions where only some root actions parry a win threatened for
the next ply) do not need the GPU.
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

DEV = "cuda:0"
M = 64
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r08", "tree_policy.json")
BUDGETS = ((64, 16), (256, 16), (256, 64), (1024, 16))  # (iterations, playouts)
CANDIDATES = 32  # gbl_playout_values at the same playouts per board: K = iterations * playouts / 32 per candidate (~30 candidates)


def states(n, dev=DEV):
    env = G.BatchedGobblet(n, dev, auto_reset=True, seed=11)
    env.rollout(64)
    if dev != "cpu":
        torch.cuda.synchronize()
    return env.squares.clone(), env.to_move.clone()


def timed(fn, iters):
    fn(0)  # warm
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for i in range(iters):
        e0.record()
        fn(1 + i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def time_tree(st, tm, I, P, explore, iters=5):
    n = st.shape[0]
    v = torch.empty((n, 54), dtype=torch.int32, device=DEV)
    w, l = torch.empty_like(v), torch.empty_like(v)
    a = torch.empty(n, dtype=torch.int32, device=DEV)
    nd, p = torch.empty_like(a), torch.empty_like(a)

    def go(call):
        nat.check(nat.lib().gbl_tree_search(st.data_ptr(), tm.data_ptr(), None, I, P, M, explore, 0, 0, call, v.data_ptr(), w.data_ptr(),
                                            l.data_ptr(), a.data_ptr(), nd.data_ptr(), p.data_ptr(), n, nat.current_stream(DEV)),
                  "gbl_tree_search")
    times = timed(go, iters)
    return times, int(p.sum()), float(nd.to(torch.float64).mean())


def time_playout(st, tm, K, iters=5):
    n = st.shape[0]
    w = torch.empty((n, 54), dtype=torch.int32, device=DEV)
    l = torch.empty_like(w)
    a = torch.empty(n, dtype=torch.int32, device=DEV)
    p = torch.empty_like(a)

    def go(call):
        nat.check(nat.lib().gbl_playout_values(st.data_ptr(), tm.data_ptr(), None, K, M, 0, 0, call, w.data_ptr(), l.data_ptr(),
                                               a.data_ptr(), p.data_ptr(), n, nat.current_stream(DEV)), "gbl_playout_values")
    return float(np.median(timed(go, iters))), int(p.sum())


def tree_waves(n, P):  # the library's rule (csrc/gobblet_hip.hip tree_waves)
    w = 1
    while w < 4 and n * (2 * w) <= 8192 and 64 * (2 * w) <= P:
        w *= 2
    return w


def arena(policy, n, seed, opponent):
    """`policy` as player_1 against `opponent` ("greedy": depth-2 greedy, or a policy object) over n games in lockstep."""
    dev = policy.device
    env = G.BatchedGobblet(n, dev, auto_reset=False, seed=seed)
    other = G.GreedyGobbletPolicy(depth=2, seed=seed, device=dev) if opponent == "greedy" else opponent
    for t in range(64):
        if bool(env.done.all()):
            break
        who = policy if t % 2 == 0 else other
        a = who.compute_actions_from_state(env.squares, env.to_move, env.action_mask)
        env.step(torch.where(env.done != 0, torch.zeros_like(a), a))
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return int((env.winner == 1).sum()), int((env.winner == -1).sum())


def merge(out_path, sections):
    rec = json.load(open(out_path)) if os.path.exists(out_path) else {}
    rec.update(sections)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", out_path)


def leaf_lane_model(cpu, st, tm, P, W):
    """Share of the lane-ply slots of k_tree's evaluation step that play a useful ply, on the leaves one ply below the root of
    the given boards: the P playouts of a leaf are dealt round-robin to the 64 W lanes, a playout of L plies takes
    ceil((L + 1) / 4) quanta of four slots (word 0 of its first Philox block belongs to the expansion), and every wavefront issues
    64 slots per slot of its busiest lane -- in the longest-running wavefront's time for all of them (the barrier).  The lengths
    come from gbl_cpu_playout_values on one candidate at a time (plies of K = k + 1 minus those of K = k, minus the root move)."""
    useful = issued = 0
    p = np.zeros(1, np.int32)
    for i in range(len(st)):
        s, m = st[i], tm[i:i + 1]
        legal = np.zeros(54, np.int8)
        assert cpu.gbl_cpu_legal_mask(s.ctypes.data, m.ctypes.data, legal.ctypes.data, 1, None) == 0
        for a in np.flatnonzero(legal):
            one = np.zeros(54, np.int8)
            one[a] = 1
            lens, prev = [], 0
            for k in range(1, P + 1):
                assert cpu.gbl_cpu_playout_values(s.ctypes.data, m.ctypes.data, one.ctypes.data, k, M, 0, 0, 0, None, None, None,
                                                  p.ctypes.data, 1, None) == 0
                lens.append(int(p[0]) - prev - 1)
                prev = int(p[0])
            if max(lens) == 0:
                continue  # (decided by the move itself: nothing is played)
            slots = np.zeros(64 * W, np.int64)
            for j, L in enumerate(lens):
                slots[j % (64 * W)] += 4 * ((L + 4) // 4)
            useful += sum(lens)
            issued += 64 * W * int(slots.max())
    return useful / max(1, issued)


def host(out_path, games=4096, threads=0):
    nat.cpu_raw().gbl_cpu_set_threads(threads)
    from tests.test_tree_policy import run, threat_positions
    from tests.test_playout_policy import run as run_mc
    sweep = []
    for explore in (0, 16, 32, 64, 128, 256, 512):
        t0 = time.time()
        pol = G.TreeSearchGobbletPolicy(iterations=256, playouts=16, max_plies=M, explore=explore, seed=0, device="cpu")
        w, l = arena(pol, games, 7, "greedy")
        sweep.append({"explore": explore, "iterations": 256, "playouts": 16, "opponent": "greedy", "games": games, "tree_wins": w,
                      "tree_losses": l, "unfinished": games - w - l, "seconds": time.time() - t0})
        print(json.dumps(sweep[-1]), flush=True)
    best = max(sweep, key=lambda r: r["tree_wins"] - r["tree_losses"])["explore"]
    st, tm, safe = threat_positions(60, seed=100)
    threat = []
    for I, P in ((64, 16), (128, 16), (256, 16), (512, 16), (1024, 16), (1024, 4), (256, 64)):
        a = run(nat.cpu_raw(), st, tm, None, I, P, M, best, 0, 0, 0)[3]
        K = max(1, I * P // CANDIDATES)
        mc = run_mc(nat.cpu_raw(), st, tm, None, K, M, 0, 0, 0)[2]
        threat.append({"iterations": I, "playouts": P, "explore": best, "positions": len(st),
                       "tree_missed": sum(int(x) not in s for x, s in zip(a, safe)), "mc_playouts_per_action": K,
                       "mc_missed": sum(int(x) not in s for x, s in zip(mc, safe))})
        print(json.dumps(threat[-1]), flush=True)
    c5s, c5m = states(64, "cpu")
    c5s, c5m = c5s.numpy()[:6].copy(), c5m.numpy()[:6].copy()
    lanes = [{"playouts": P, "waves_per_board": W, "useful_share_of_lane_slots": leaf_lane_model(nat.cpu_raw(), c5s, c5m, P, W)}
             for P, W in ((16, 1), (64, 1), (256, 1), (256, 4))]
    print(json.dumps(lanes), flush=True)
    merge(out_path, {"explore_sweep": sweep, "explore_default": best, "threat": threat, "leaf_lane_model": lanes})


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--trace"]:
        n, I, P = (int(x) for x in argv[1:4])
        st, tm = states(n)
        times, plies, nodes = time_tree(st, tm, I, P, 128, 3)
        ms = float(np.median(times))
        print(json.dumps({"boards": n, "iterations": I, "playouts": P, "ms": ms, "plies": plies}))
        return
    if argv[:1] == ["--host"]:
        host(argv[1] if len(argv) > 1 else DEFAULT_OUT)
        return
    out_path = argv[0] if argv else DEFAULT_OUT
    explore = G.TreeSearchGobbletPolicy(device="cpu").explore  # the default
    rows = []
    for n in (4096, 65536):
        st, tm = states(n)
        for I, P in BUDGETS:
            times, plies, nodes = time_tree(st, tm, I, P, explore)
            ms = float(np.median(times))
            K = I * P // CANDIDATES
            pms, pplies = time_playout(st, tm, K, 3)
            rate, prate = plies / (ms / 1e3), pplies / (pms / 1e3)
            rows.append({"boards": n, "iterations": I, "playouts": P, "max_plies": M, "explore": explore,
                         "waves_per_board": tree_waves(n, P), "ms_per_launch": ms, "ms_min": min(times), "ms_max": max(times), "decisions_per_s": n / (ms / 1e3),
                         "useful_plies_per_s": rate, "plies_per_decision": plies / n, "nodes_per_decision": nodes,
                         "playout_values_playouts": K, "playout_values_ms": pms, "playout_values_plies_per_s": prate,
                         "plies_per_s_vs_playout_values": rate / prate})
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    games, arenas = 4096, []

    def tree(I, P):
        return G.TreeSearchGobbletPolicy(iterations=I, playouts=P, max_plies=M, explore=explore, seed=0, device=DEV)
    pairs = [((64, 16), "greedy"), ((256, 16), "greedy"), ((1024, 16), "greedy"), ((64, 16), 32), ((256, 16), 128), ((256, 64), 512),
             ((1024, 16), 512)]
    for (I, P), opp in pairs:
        t0 = time.time()
        other = opp if opp == "greedy" else G.MonteCarloGobbletPolicy(playouts=opp, max_plies=M, seed=1, device=DEV)
        w, l = arena(tree(I, P), games, 7, other)
        arenas.append({"iterations": I, "playouts": P, "tree_playouts_per_decision": I * P,
                       "opponent": opp if opp == "greedy" else f"mc({opp})", "games": games, "tree_wins": w, "tree_losses": l,
                       "unfinished": games - w - l, "seconds": time.time() - t0})
        print(json.dumps(arenas[-1]), flush=True)
    # the same pairings with the sides swapped (flat Monte-Carlo as player_1): the first mover's advantage is not the tree's
    for (I, P), K in (((256, 16), 128), ((1024, 16), 512)):
        t0 = time.time()
        w, l = arena(G.MonteCarloGobbletPolicy(playouts=K, max_plies=M, seed=1, device=DEV), games, 7, tree(I, P))
        arenas.append({"iterations": I, "playouts": P, "tree_playouts_per_decision": I * P, "opponent": f"mc({K}) as player_1",
                       "games": games, "tree_wins": l, "tree_losses": w, "unfinished": games - w - l, "seconds": time.time() - t0})
        print(json.dumps(arenas[-1]), flush=True)
    merge(out_path, {"metric": "gbl_tree_search: leaf-parallel UCT (k_tree), M = 64, BASELINE config 5 states",
                     "device": torch.cuda.get_device_name(0), "rows": rows, "arena": arenas})


if __name__ == "__main__":
    main()
