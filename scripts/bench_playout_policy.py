#!/usr/bin/env python3
"""gbl_playout_values (MonteCarloGobbletPolicy) on the GPU: decisions/s, useful plies/s and lane utilisation at N x K, M = 64, on
the stationary masked-random mix (BatchedGobblet(N, seed=11).rollout(64), as BASELINE config 5), plus an arena of MC(K) as
player_1 against the masked-random player and depth-2 greedy.

    python scripts/bench_playout_policy.py [out.json]            (default: profiles/r07/playout_policy.json)
    python scripts/bench_playout_policy.py --trace N K           (one warm launch + 3 timed ones, for rocprofv3 runs)

useful plies = sum of plies_out (every ply a playout played, root moves included).  Lane utilisation = useful plies / lane-ply
slots the kernel issues, from a model of k_playout's schedule on the exact playout lengths of a sample of boards: items are dealt
round-robin to the 64 W lanes of a board, a lane spends ceil(L / 4) quanta of four plies on a playout of L plies, and a
wavefront issues 64 slots per ply of its busiest lane.  The per-playout lengths come from the host flavour (the plies of K = k + 1
minus those of K = k, one candidate at a time).
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
ROLLOUT_PLIES_PER_S = 1.846e11  # profiles/r06/playouts.json: gbl_rollout, 2^20 boards x 64 plies per launch


def states(n):
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=11)
    env.rollout(64)
    torch.cuda.synchronize()
    return env.squares.clone(), env.to_move.clone()


def launch(st, tm, K, out, call=0):
    w, l, a, p = out
    nat.check(nat.lib().gbl_playout_values(st.data_ptr(), tm.data_ptr(), None, K, M, 0, 0, call, w.data_ptr(), l.data_ptr(),
                                           a.data_ptr(), p.data_ptr(), st.shape[0], nat.current_stream(DEV)), "gbl_playout_values")


def outputs(n):
    return (torch.empty((n, 54), dtype=torch.int32, device=DEV), torch.empty((n, 54), dtype=torch.int32, device=DEV),
            torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV))


def time_ms(st, tm, K, iters):
    out = outputs(st.shape[0])
    launch(st, tm, K, out)  # warm
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for i in range(iters):
        e0.record()
        launch(st, tm, K, out, call=1 + i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), int(out[3].sum())


def waves_of(n, K):  # the library's rule (csrc/gobblet_hip.hip playout_waves)
    w = 1
    while w < 8 and n * (2 * w) <= 16384 and 64 * (2 * w) * 4 <= 30 * K:
        w *= 2
    return w


def playout_lengths(cpu, s, m, K):
    """Plies of every playout of one board, in item order (rank-major: item = rank * K + k)."""
    legal = np.zeros(54, np.int8)
    assert cpu.gbl_cpu_legal_mask(s.ctypes.data, m.ctypes.data, legal.ctypes.data, 1, None) == 0
    lens = []
    p = np.zeros(1, np.int32)
    for a in np.flatnonzero(legal):
        one = np.zeros(54, np.int8)
        one[a] = 1
        prev = 0
        for k in range(1, K + 1):
            assert cpu.gbl_cpu_playout_values(s.ctypes.data, m.ctypes.data, one.ctypes.data, k, M, 0, 0, 0, None, None, None,
                                              p.ctypes.data, 1, None) == 0
            lens.append(int(p[0]) - prev)
            prev = int(p[0])
    return np.array(lens)


def lane_model(lens, W):
    lanes = 64 * W
    slots = np.zeros(lanes, np.int64)
    for i, L in enumerate(lens):
        slots[i % lanes] += 4 * ((L + 3) // 4)
    issued = sum(64 * int(slots[64 * w: 64 * (w + 1)].max()) for w in range(W))
    return float(lens.sum()) / max(1, issued)


def arena(policy, n, seed, opponent):
    env = G.BatchedGobblet(n, DEV, auto_reset=False, seed=seed)
    other = G.GreedyGobbletPolicy(depth=2, seed=seed, device=DEV) if opponent == "greedy" else None
    for t in range(64):
        if bool(env.done.all()):
            break
        if t % 2 == 0:
            a = policy.compute_actions_from_state(env.squares, env.to_move, env.action_mask)
        elif other is not None:
            a = other.compute_actions_from_state(env.squares, env.to_move, env.action_mask)
        else:
            a = env.sample_actions()
        env.step(torch.where(env.done != 0, torch.zeros_like(a), a))
    torch.cuda.synchronize()
    return int((env.winner == 1).sum()), int((env.winner == -1).sum())


def main():
    if sys.argv[1:2] == ["--trace"]:
        n, K = int(sys.argv[2]), int(sys.argv[3])
        st, tm = states(n)
        ms, plies = time_ms(st, tm, K, 3)
        print(json.dumps({"boards": n, "playouts": K, "ms": ms, "plies": plies}))
        return
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r07", "playout_policy.json")
    cpu = nat.cpu_raw()
    cpu.gbl_cpu_set_threads(16)
    sample_st, sample_tm = None, None
    rows = []
    for n in (4096, 65536):
        st, tm = states(n)
        if sample_st is None:
            sample_st, sample_tm = st[:6].cpu().numpy().copy(), tm[:6].cpu().numpy().copy()
        for K in (16, 64, 256):
            ms, plies = time_ms(st, tm, K, 5 if K < 256 else 3)
            W = waves_of(n, K)
            util = [lane_model(playout_lengths(cpu, sample_st[i], sample_tm[i:i + 1], K), W) for i in range(len(sample_st))]
            rows.append({"boards": n, "playouts": K, "max_plies": M, "waves_per_board": W, "ms_per_launch": ms,
                         "decisions_per_s": n / (ms / 1e3), "useful_plies_per_s": plies / (ms / 1e3),
                         "plies_per_decision": plies / n, "vs_rollout": plies / (ms / 1e3) / ROLLOUT_PLIES_PER_S,
                         "lane_utilisation_model": float(np.mean(util))})
            print(json.dumps(rows[-1]), flush=True)
            torch.cuda.empty_cache()
    games = 4096
    arenas = []
    for K in (16, 64, 256):
        for opp in ("random", "greedy"):
            t0 = time.time()
            w, l = arena(G.MonteCarloGobbletPolicy(playouts=K, max_plies=M, seed=0, device=DEV), games, 7, opp)
            arenas.append({"mc_playouts": K, "opponent": opp, "games": games, "mc_wins": w, "mc_losses": l,
                           "unfinished": games - w - l, "seconds": time.time() - t0})
            print(json.dumps(arenas[-1]), flush=True)
    rec = {"metric": "gbl_playout_values: flat Monte-Carlo playout values (k_playout), M = 64, BASELINE config 5 states",
           "device": torch.cuda.get_device_name(0), "rollout_reference_plies_per_s": ROLLOUT_PLIES_PER_S, "rows": rows,
           "arena": arenas}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
