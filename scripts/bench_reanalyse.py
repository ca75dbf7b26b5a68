#!/usr/bin/env python3
"""gbl_reanalyse on one MI355X beside the composition it replaces -- gbl_decode_obs into temporaries, gbl_tree_search_eval, the torch
narrowing from int32 to int16 and the (strided) copy into the visits rows -- in the same process, alternating.  HIP events, one
warm-up, the median of five (scripts/bench_training_batch.py's timed_pair).  H = 64 (seeded integer weights), 64 iterations, explore 16.
Three parts, each a process of its own (run each under its own `timeout`, chained with &&); each merges its section into the record:

    python scripts/bench_reanalyse.py kernel [out.json]   4 096 and 65 536 rows of the masked-random mix (seed 11, 64 plies), a batch's
                                                          pitches, visits and drift out
    python scripts/bench_reanalyse.py ring   [out.json]   a ring of 2^20 live rows (a 65 536-board x 32-ply window of tree-against-tree
                                                          self-play, wrapped) in place through the ring's pitches
    python scripts/bench_reanalyse.py fit    [out.json]   one step of ReplayBuffer.fit at batch 1 024 with and without reanalyse=

Default record: profiles/r27/reanalyse.json.  Recorded numbers, no gate (tests/test_gpu_reanalyse_guard.py asserts its own ratio).
With GOBBLET_HIP_LIB=build/lib_NAME.so the parts run on an experiment build (scripts/build_variant.sh NAME -DGBL_REANALYSE_GROUPS=n:
another grid cap; the record's `grid_caps` section is the ring part of four such builds)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_solver as BS  # noqa: E402  (merge)
import bench_training_batch as B  # noqa: E402  (the window, timed_pair, stats)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

DEV = B.DEV
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r27", "reanalyse.json")
ITERATIONS, EXPLORE, HIDDEN = 64, 16, 64


def evaluator():
    rng = np.random.default_rng(0)
    return G.GobbletEvaluator(rng.integers(-128, 128, (117, HIDDEN), dtype=np.int8), rng.integers(-300, 300, HIDDEN),
                              rng.integers(-128, 128, (HIDDEN // 4, 56, 4), dtype=np.int8), rng.integers(-65536, 65536, 56), 1, 9, 9, device=DEV)


def mix_rows(n):
    """n observation rows and masks of the masked-random mix (seed 11, 64 plies)."""
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=11)
    env.rollout(64)
    torch.cuda.synchronize()
    return env.observation.reshape(n, nat.OBS_BYTES).clone(), env.action_mask.clone()


def launchers(ev, n, obs, obs_pitch, mask, mask_pitch, visits_rows, visits_pitch, z, z_pitch, drift=True):
    """Two callables on the same n pitched rows: the fused launch (in place where visits_rows holds the old visits) and the
    composition.  visits_rows: an int16 (n, 54) view of the destination (a batch's tensor, or the ring's rows without the padding)."""
    lib, s = nat.lib(), nat.current_stream(DEV)
    state, who = torch.empty((n, nat.CELLS), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)
    wide = torch.empty((n, nat.ACTIONS), dtype=torch.int32, device=DEV)
    moved = torch.empty(n, dtype=torch.int32, device=DEV) if drift else None
    dense = obs_pitch == nat.OBS_BYTES
    packed_obs = None if dense else torch.empty((n, nat.OBS_BYTES), dtype=torch.int8, device=DEV)
    packed_mask = None if dense else torch.empty((n, nat.ACTIONS), dtype=torch.int8, device=DEV)
    struct = ev.as_struct()

    def fused():
        nat.check(lib.gbl_reanalyse(C.addressof(struct), ITERATIONS, EXPLORE, obs.data_ptr(), obs_pitch, mask.data_ptr(), mask_pitch,
                                    visits_rows.data_ptr(), visits_rows.data_ptr(), visits_pitch, nat.ptr(z), z_pitch, None, None, None, None,
                                    nat.ptr(moved), None, n, s), "gbl_reanalyse")

    def composition():
        o, m = obs, mask
        if not dense:  # (gbl_decode_obs and gbl_tree_search_eval take dense rows: the ring's pitched ones are packed first)
            packed_obs.copy_(obs[:, :nat.OBS_BYTES])
            packed_mask.copy_(mask[:, :nat.ACTIONS])
            o, m = packed_obs, packed_mask
        nat.check(lib.gbl_decode_obs(o.data_ptr(), state.data_ptr(), who.data_ptr(), n, s), "gbl_decode_obs")
        nat.check(lib.gbl_tree_search_eval(state.data_ptr(), who.data_ptr(), m.data_ptr(), C.addressof(struct), ITERATIONS, EXPLORE, wide.data_ptr(),
                                           None, None, None, None, None, None, n, s), "gbl_tree_search_eval")
        visits_rows.copy_(wide)  # (the narrowing and, for the ring, the strided scatter; no drift)

    return fused, composition


def pair(n):
    """The two callables at n rows of the mix with a batch's pitches: the kernel part's and the guard's."""
    ev = evaluator()
    obs, mask = mix_rows(n)
    visits = torch.zeros((n, nat.ACTIONS), dtype=torch.int16, device=DEV)
    fused, composition = launchers(ev, n, obs, nat.OBS_BYTES, mask, nat.ACTIONS, visits, nat.ACTIONS, None, 1)
    fused()
    mine = visits.clone()
    visits.zero_()
    composition()
    torch.cuda.synchronize()
    assert torch.equal(mine, visits), "the kernel and the composition disagree"
    return {"gbl_reanalyse": fused, "decode_obs + tree_search_eval + torch": composition}, (ev, obs, mask, visits)


def kernel(path):
    rows = []
    for n in (4096, 65536):
        fns, keep = pair(n)
        row = {"rows": n, **{k: B.stats(v) for k, v in B.timed_pair(fns).items()}}
        print(json.dumps(row), flush=True)
        rows.append(row)
    BS.merge(path, "kernel", {"device": torch.cuda.get_device_name(0), "hidden": HIDDEN, "iterations": ITERATIONS, "explore": EXPLORE, "rows": rows})


def selfplay_ring(capacity):
    env, traj = B.window()
    buf = G.ReplayBuffer(capacity, DEV)
    buf.append(env, traj)
    torch.cuda.synchronize()
    return buf


def ring(path):
    ev, buf = evaluator(), selfplay_ring(1 << 20)
    live = buf.size
    assert live == 1 << 20
    fused, composition = launchers(ev, live, buf._obs, nat.REPLAY_OBS_PITCH, buf._meta, nat.REPLAY_META_PITCH, buf.visits, nat.REPLAY_VISITS_PITCH,
                                   buf.z, nat.REPLAY_META_PITCH)
    t = B.timed_pair({"gbl_reanalyse, in place": fused, "pack + decode_obs + tree_search_eval + torch scatter": composition,
                      "ReplayBuffer.reanalyse": lambda: buf.reanalyse(ev, ITERATIONS, EXPLORE)})
    rec = {"ring_rows": live, "ring_bytes": live * 320, **{k: B.stats(v) for k, v in t.items()}}
    print(json.dumps(rec), flush=True)
    BS.merge(path, "ring_in_place", rec)


def fit(path):
    ev, buf = evaluator(), selfplay_ring(1 << 20)
    a, b = G.GobbletTrainer(hidden=64, device=DEV, seed=0), G.GobbletTrainer(hidden=64, device=DEV, seed=0)
    spec = dict(evaluator=ev, iterations=ITERATIONS, explore=EXPLORE)
    t = B.timed_pair({"fit step, plain": lambda: buf.fit(a, 1, batch=1024), "fit step, reanalyse=": lambda: buf.fit(b, 1, batch=1024, reanalyse=spec)})
    rec = {"batch": 1024, "hidden": 64, **{k: B.stats(v) for k, v in t.items()}}
    print(json.dumps(rec), flush=True)
    BS.merge(path, "fit_step", rec)


if __name__ == "__main__":
    {"kernel": kernel, "ring": ring, "fit": fit}[sys.argv[1]](sys.argv[2] if len(sys.argv) > 2 else DEFAULT_OUT)
