#!/usr/bin/env python3
"""Prioritised replay on the GPU: HIP events, one warm-up, the median of five, everything in one process, alternating.

    python scripts/bench_replay_prio.py [out.json]      (default: profiles/r25/replay_prio.json)

On a ring of 2^21 slots of random rows with random priorities in 1 .. 1 000, at batch 65 536:
(a) the index build plus gbl_replay_batch_prio against the torch composition it replaces on the same ring: torch.cumsum of the
    priorities as int64, torch.searchsorted of 65 536 targets (drawn beforehand) and gbl_replay_batch standing in for the row gathers --
    what tests/test_gpu_replay_prio_guard.py gates at 1.0 x;
(b) gbl_replay_batch_prio alone against gbl_replay_batch alone, and the build alone;
(c) a fit step at H = 64, batch 4 096, with and without prioritized=True (the build is not repeated: nothing changes between steps).
And on a 4 096-board x 32-ply window of tree-against-tree self-play:
(d) gbl_replay_prio_append beside the gbl_replay_append it follows.
GOBBLET_HIP_LIB=build/lib_NAME.so times an experiment build."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_training_batch as B  # noqa: E402  (the timing)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

DEV = B.DEV
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r25", "replay_prio.json")
SLOTS, BATCH, FIT_BATCH = 1 << 21, 65536, 4096
APPEND_BOARDS, APPEND_PLIES = 4096, 32


def random_ring(slots=SLOTS, seed=1):
    """A full prioritised ring of random rows (observations of 0 / 1 bytes, mover bytes 0 / 1) with priorities in 1 .. 1 000."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = G.ReplayBuffer(slots, DEV, prioritized=True)
    buf._obs[:, :nat.OBS_BYTES] = torch.randint(0, 2, (slots, nat.OBS_BYTES), device=DEV, generator=g, dtype=torch.int8)
    buf._visits[:, :nat.ACTIONS] = torch.randint(0, 64, (slots, nat.ACTIONS), device=DEV, generator=g, dtype=torch.int16)
    buf._meta[:, :nat.ACTIONS + 2] = torch.randint(0, 2, (slots, nat.ACTIONS + 2), device=DEV, generator=g, dtype=torch.int8)
    buf._state[0] = slots
    buf.set_all_priority(torch.randint(1, 1001, (slots,), device=DEV, generator=g, dtype=torch.int32))
    torch.cuda.synchronize()
    return buf


def launchers(buf, batch=BATCH):
    """The callables that are timed, each drawing call = 1, 2, ... into its own reused outputs."""
    uniform_out, prio_out = buf.batch(batch), buf.batch(batch, prioritized=True)
    total = int(buf.priority.to(torch.int64).sum())
    targets = torch.randint(0, total, (batch,), device=DEV, dtype=torch.int64)
    call = [0]

    def uniform():
        call[0] += 1
        buf.batch(batch, call=call[0], out=uniform_out)

    def draw():   # (the index is current: gbl_replay_batch_prio alone)
        call[0] += 1
        buf.batch(batch, call=call[0], out=prio_out, prioritized=True)

    def build():
        buf._index_current = False
        buf._rebuild_index()

    def build_and_draw():
        buf._index_current = False
        draw()

    def composition():
        cum = torch.cumsum(buf.priority, 0, dtype=torch.int64)
        torch.searchsorted(cum, targets, right=True)
        uniform()

    return {"build_and_draw": build_and_draw, "composition": composition, "batch_prio": draw, "batch": uniform, "build": build}


def guard_pair(buf):
    """(index build + gbl_replay_batch_prio, the torch composition) in microseconds: medians of five, alternating."""
    L = launchers(buf)
    t = B.timed_pair({k: L[k] for k in ("build_and_draw", "composition")})
    return tuple(1e3 * float(np.median(t[k])) for k in ("build_and_draw", "composition"))


def bench_draw(buf):
    L = launchers(buf)
    rec = {k: B.stats(v) for k, v in B.timed_pair(L).items()}
    rec["composition_over_build_and_draw"] = rec["composition"]["median_us"] / rec["build_and_draw"]["median_us"]
    rec["batch_prio_over_batch"] = rec["batch_prio"]["median_us"] / rec["batch"]["median_us"]
    return rec


def bench_fit(buf):
    trainers = {k: G.GobbletTrainer(hidden=64, device=DEV, seed=1) for k in ("uniform", "prioritized")}
    call = [0]

    def step(name):
        def fn():
            call[0] += 1
            buf.fit(trainers[name], 1, batch=FIT_BATCH, first_call=call[0], prioritized=name == "prioritized")
        return fn
    return {"batch": FIT_BATCH, "hidden": 64, **{k: B.stats(v) for k, v in B.timed_pair({k: step(k) for k in trainers}).items()}}


def bench_append():
    env = G.BatchedGobblet(APPEND_BOARDS, DEV, auto_reset=True, seed=5, track_turn=True)
    traj = env.collect(APPEND_PLIES, policies=("tree", "tree"), search=B.SEARCH, out="fresh")
    env.outcome_targets(traj)
    cells = (APPEND_PLIES - 1) * APPEND_BOARDS
    plain, prio = G.ReplayBuffer(cells, DEV), G.ReplayBuffer(cells, DEV, prioritized=True)
    per_cell = torch.randint(0, 16, traj["z"].shape, device=DEV, dtype=torch.int32)
    t = B.timed_pair({"append": lambda: plain.append(env, traj, tag=1), "append_and_prio_append": lambda: prio.append(env, traj, tag=1, priority=3),
                      "append_and_prio_append_per_cell": lambda: prio.append(env, traj, tag=1, priority=per_cell)})
    return {"boards": APPEND_BOARDS, "plies": APPEND_PLIES, "valid_rows": plain.total // 6, **{k: B.stats(v) for k, v in t.items()},
            "per_cell_note": "the per-cell form includes the torch copy of the priorities into the window's strides"}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    buf = random_ring()
    rec = {"device": torch.cuda.get_device_name(0), "timing": "HIP events, one warm-up, five repetitions alternating",
           "ring": {"slots": SLOTS, "priorities": "uniform in 1 .. 1000", "index_bytes": nat.lib().gbl_replay_prio_index_bytes(SLOTS)},
           "batch": BATCH, "draw": bench_draw(buf), "fit_step": bench_fit(buf), "append": bench_append()}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
