#!/usr/bin/env python3
"""The replay buffer on the GPU: HIP events, one warm-up, the median of five, everything in one process, alternating.

    python scripts/bench_replay.py [out.json]      (default: profiles/r21/replay.json)

(a) gbl_replay_batch at batch 4 096 and 65 536 from the ring that one 65 536-board x 32-ply window of tree-vs-tree self-play was
    appended to, against gbl_training_batch on that same window (scripts/bench_training_batch.py's window and launcher).
(b) gbl_replay_append of that window -- its three launches together -- with the fraction of 8 TB/s on the bytes it must move:
        cells x (1 + 1 + 108)           z, done and the visits row of every cell, read once by the count (the scatter reads the ballots)
      + chunks x 40                     a chunk's ballot written and read twice, its base written and read
      + K x (117 + 54 + 108 + 2)        the valid rows' observation, mask, visits, z and mover, read by the scatter
      + K x (128 + 128 + 64)            the ring rows written
    and beside it the torch composition it replaces: a boolean keep mask, nonzero(), three index_select()s (and two for z and the
    mover) and the index_copy_()s into a ring of the same pitches.
GOBBLET_HIP_LIB=build/lib_NAME.so times an experiment build."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_training_batch as B  # noqa: E402  (the window, the sampler's launcher, the timing)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

DEV = B.DEV
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r21", "replay.json")
BATCHES = (4096, 65536)


def filled_buffer(env, traj):
    """A ring with a slot for every cell of the window, the window appended once."""
    buf = G.ReplayBuffer((traj["_plies"] - 1) * env.num_envs, DEV)
    buf.append(env, traj, tag=1)
    torch.cuda.synchronize()
    return buf


def replay_launcher(buf, batch):
    """A callable that draws the next batch (call = 1, 2, ...) into one set of output tensors."""
    out = buf.batch(batch)
    call = [0]

    def kernel():
        call[0] += 1
        buf.batch(batch, call=call[0], out=out)
    return kernel


def bench_batch(env, traj, buf):
    rows = []
    for batch in BATCHES:
        sampler, _ = B.kernel_launcher(env, traj, batch)
        t = B.timed_pair({"replay": replay_launcher(buf, batch), "window": sampler})
        row = {"batch": batch, "replay_batch": B.stats(t["replay"]), "training_batch": B.stats(t["window"])}
        row["training_batch_over_replay_batch"] = row["training_batch"]["median_us"] / row["replay_batch"]["median_us"]
        row.update(replay_lines_bytes_per_sample=128 + 128 + 64, output_bytes_per_sample=117 + 54 + 108 + 1 + 8 + 2)
        rows.append(row)
    return rows


def bench_append(env, traj, buf):
    n, plies = env.num_envs, traj["_plies"]
    cells, chunks, K = (plies - 1) * n, (plies - 1) * -(-n // 64), buf.total
    obs_w, mask_w = traj["observation"][:-1].reshape(cells, 117), traj["action_mask"][:-1].reshape(cells, 54)
    visits_w, z_w, done_w, mover_w = traj["visits"][1:].reshape(cells, 54), traj["z"][1:].reshape(cells), traj["done"][:-1].reshape(cells), \
        traj["mover"][1:].reshape(cells)
    cap = buf.capacity
    ring = {"obs": torch.zeros((cap, 128), dtype=torch.int8, device=DEV), "visits": torch.zeros((cap, 64), dtype=torch.int16, device=DEV),
            "meta": torch.zeros((cap, 64), dtype=torch.int8, device=DEV)}
    pos = [0]

    def compose():
        keep = (z_w != nat.Z_OPEN) & (done_w == 0) & (visits_w.sum(-1, dtype=torch.int32) > 0)
        idx = keep.nonzero().squeeze(1)
        slots = (pos[0] + torch.arange(len(idx), device=DEV)) % cap
        ring["obs"][:, :117].index_copy_(0, slots, obs_w.index_select(0, idx))
        ring["visits"][:, :54].index_copy_(0, slots, visits_w.index_select(0, idx))
        ring["meta"][:, :54].index_copy_(0, slots, mask_w.index_select(0, idx))
        ring["meta"][:, 54].index_copy_(0, slots, z_w.index_select(0, idx))
        ring["meta"][:, 55].index_copy_(0, slots, mover_w.index_select(0, idx))
        pos[0] += len(idx)

    t = B.timed_pair({"append": lambda: buf.append(env, traj, tag=2), "torch": compose})
    moved = cells * 110 + chunks * 40 + K * (117 + 54 + 108 + 2) + K * (128 + 128 + 64)
    rec = {"append": B.stats(t["append"]), "torch_composition": B.stats(t["torch"]), "cells": cells, "chunks": chunks, "valid_rows": K,
           "bytes_moved": moved,
           "bytes_formula": "cells * (1 + 1 + 108) + chunks * 40 + K * (117 + 54 + 108 + 2) + K * (128 + 128 + 64)"}
    rec["fraction_of_8_TB_s"] = moved / (rec["append"]["median_us"] * 1e-6) / B.HBM_BYTES_PER_S
    rec["torch_over_append"] = rec["torch_composition"]["median_us"] / rec["append"]["median_us"]
    return rec


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    env, traj = B.window()
    buf = filled_buffer(env, traj)
    rec = {"device": torch.cuda.get_device_name(0), "timing": "HIP events, one warm-up, five repetitions alternating",
           "window": {"boards": env.num_envs, "plies": traj["_plies"], "layout": "time", "search": B.SEARCH,
                      "valid_share": buf.total / ((traj["_plies"] - 1) * env.num_envs)},
           "ring": {"capacity": buf.capacity, "bytes_per_row": 320},
           "batch": bench_batch(env, traj, buf), "append": bench_append(env, traj, buf)}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
