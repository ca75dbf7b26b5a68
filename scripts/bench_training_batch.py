#!/usr/bin/env python3
"""gbl_symmetry_apply and gbl_training_batch on the GPU: HIP events, one warm-up, the median of five.

    python scripts/bench_training_batch.py [out.json]      (default: profiles/r15/training_batch.json)

(a) gbl_symmetry_apply with all six row types at 2^20 boards: microseconds and the fraction of 8 TB/s on its algorithmic bytes,
    2 x (27 + 117 + 54 + 108 + 54 + 4) + 3 per board.
(b) gbl_training_batch at batch 4 096 and 65 536 from a 65 536-board x 32-ply time-major window of tree-vs-tree self-play, against the
    torch composition it replaces, on the same device in the same process, alternating: the boolean masks and nonzero() of
    examples/example_train_evaluator.py's targets_of, torch.randint, row gathers, and the symmetry as gathers through precomputed
    index tables.  The composition is timed twice: as written (the keep set rebuilt for every batch, as a trainer that streams new
    windows does) and with the keep set built once outside the timed region.  Also the bytes of 128-byte lines a sample touches.
GOBBLET_HIP_LIB=build/lib_NAME.so times an experiment build."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402
from gobblet_rl_amd import symmetry as S  # noqa: E402

if os.environ.get("GOBBLET_HIP_LIB"):
    nat.use_library(os.environ["GOBBLET_HIP_LIB"])

DEV = "cuda:0"
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r15", "training_batch.json")
HBM_BYTES_PER_S = 8e12
APPLY_BOARDS, APPLY_BYTES = 1 << 20, 2 * (27 + 117 + 54 + 108 + 54 + 4) + 3
WINDOW_BOARDS, WINDOW_PLIES, BATCHES = 65536, 32, (4096, 65536)
SEARCH = dict(iterations=8, playouts=2, sample_plies=4)


def timed_pair(fns, iters=5):
    """{name: [ms] * iters} of several callables, one warm-up each, then alternating."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return times


def stats(ms):
    return {"min_us": 1e3 * min(ms), "median_us": 1e3 * float(np.median(ms)), "max_us": 1e3 * max(ms)}


def bench_apply():
    n = APPLY_BOARDS
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=11)
    env.rollout(16)
    g = torch.Generator(device=DEV).manual_seed(1)
    rows = dict(state=env.squares, observation=env.observation.reshape(n, 117), action_mask=env.action_mask,
                visits=torch.randint(0, 1024, (n, 54), device=DEV, generator=g).to(torch.int16),
                priors=torch.randint(0, 256, (n, 54), device=DEV, generator=g).to(torch.uint8), actions=env.actions)
    sym = torch.randint(0, 512, (n,), device=DEV, generator=g).to(torch.int16)
    outs = {k: torch.empty_like(v) for k, v in rows.items()}
    lib, pairs = nat.lib(), []
    for k in ("state", "observation", "action_mask", "visits", "priors", "actions"):
        pairs += [rows[k].data_ptr(), outs[k].data_ptr()]

    def launch():
        nat.check(lib.gbl_symmetry_apply(sym.data_ptr(), 0, env.to_move.data_ptr(), *pairs, n, nat.current_stream(DEV)))
    rec = stats(timed_pair({"apply": launch})["apply"])
    rec.update(boards=n, bytes_per_board=APPLY_BYTES, fraction_of_8_TB_s=n * APPLY_BYTES / (rec["median_us"] * 1e-6) / HBM_BYTES_PER_S)
    return rec


def source_tables():
    """Gather tables of the 512 codes for either agent: out[k] = in[table[s, m, k]] (the inverse of symmetry.action_map and of the
    observation's byte map)."""
    act, obs = np.zeros((512, 2, 54), np.int64), np.zeros((512, 2, 117), np.int64)
    for s in range(512):
        sigma = S.position_map(s)
        for m in (0, 1):
            to = np.array(S.action_map(s, m))
            act[s, m, to] = np.arange(54)
            mine, theirs = S.piece_map(s, m), S.piece_map(s, 1 - m)
            for p in range(9):
                for ch in range(13):
                    c = mine[ch + 1] - 1 if ch < 6 else 6 + theirs[ch - 5] - 1 if ch < 12 else 12
                    obs[s, m, 13 * sigma[p] + c] = 13 * p + ch
    return torch.from_numpy(act).to(DEV), torch.from_numpy(obs).to(DEV)


def window():
    """(env, traj): the 65 536-board x 32-ply time-major window of tree-against-tree self-play with outcome targets."""
    env = G.BatchedGobblet(WINDOW_BOARDS, DEV, auto_reset=True, seed=5, track_turn=True)
    traj = env.collect(WINDOW_PLIES, policies=("tree", "tree"), search=SEARCH, out="fresh")
    env.outcome_targets(traj)
    torch.cuda.synchronize()
    return env, traj


def kernel_launcher(env, traj, batch):
    """A callable that draws the next batch (call = 1, 2, ...) into one set of output tensors, and those tensors."""
    out = env.training_batch(traj, batch)
    call = [0]

    def kernel():
        call[0] += 1
        env.training_batch(traj, batch, call=call[0], out=out)
    return kernel, out


def bench_batch():
    n, plies = WINDOW_BOARDS, WINDOW_PLIES
    env, traj = window()
    act_src, obs_src = source_tables()
    obs_w, mask_w = traj["observation"][:-1].reshape(plies - 1, n, 117), traj["action_mask"][:-1]
    visits_w, z_w, done_w, mover_w = traj["visits"][1:], traj["z"][1:], traj["done"][:-1], traj["mover"][1:]

    def keep_set():
        return ((z_w != nat.Z_OPEN) & (done_w == 0) & (visits_w.sum(-1, dtype=torch.int32) > 0)).nonzero()

    def compose(batch, cells):
        r = torch.randint(0, len(cells), (batch,), device=DEV)
        t, b = cells[r].T
        m = mover_w[t, b].long()
        s = torch.randint(0, 512, (batch,), device=DEV)
        a_src, o_src = act_src[s, m], obs_src[s, m]
        return (obs_w[t, b].gather(1, o_src), mask_w[t, b].gather(1, a_src), visits_w[t, b].gather(1, a_src), z_w[t, b],
                torch.stack([t + 1, b], 1).int(), s.to(torch.int16))

    cached = keep_set()
    rows = []
    for batch in BATCHES:
        kernel, out = kernel_launcher(env, traj, batch)
        t = timed_pair({"kernel": kernel, "torch": lambda: compose(batch, keep_set()), "torch_keep_cached": lambda: compose(batch, cached)})
        row = {"batch": batch, "kernel": stats(t["kernel"]), "torch_composition": stats(t["torch"]),
               "torch_composition_keep_set_cached": stats(t["torch_keep_cached"])}
        row["torch_over_kernel"] = row["torch_composition"]["median_us"] / row["kernel"]["median_us"]
        row["torch_keep_cached_over_kernel"] = row["torch_composition_keep_set_cached"]["median_us"] / row["kernel"]["median_us"]
        # the 128-byte lines of the rows a sample returns (its successful attempt; a failed attempt adds three scalar lines and up to
        # two of the visits row): the observation and mask rows of cell(t - 1, b), the visits row, z, done and mover of cell(t, b)
        idx = out["index"].long()
        ok = idx[:, 0] >= 0
        t_, b_ = idx[ok].T
        at, prev = t_ * traj["_ply_stride"] + b_, (t_ - 1) * traj["_ply_stride"] + b_
        lines = lambda first, size: (first + size - 1) // 128 - first // 128 + 1  # noqa: E731
        touched = lines(prev * 117, 117) + lines(prev * 54, 54) + lines(at * 108, 108) + 3
        row.update(failed_samples=int((~ok).sum()), lines_bytes_per_sample=float(128 * touched.float().mean()),
                   output_bytes_per_sample=117 + 54 + 108 + 1 + 8 + 2)
        rows.append(row)
    return {"window": {"boards": n, "plies": plies, "layout": "time", "search": SEARCH, "valid_share": len(cached) / ((plies - 1) * n)},
            "rows": rows}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    rec = {"device": torch.cuda.get_device_name(0), "timing": "HIP events, one warm-up, five repetitions alternating",
           "symmetry_apply": bench_apply(), "training_batch": bench_batch()}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
