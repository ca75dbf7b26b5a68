#!/usr/bin/env python3
"""gbl_tb_targets on one MI355X: the kernel beside the composition it replaces, the ring's relabel, a fit step with and without exact
targets, the census of a self-play ring against the truth, and the two networks of examples/example_train_tablebase.py.  HIP events,
one warm-up, the median of five (scripts/bench_tablebase.py's way).  Six parts, each a process of its own (run each under its own
`timeout`, chained with &&); every part that needs the full table builds its own (under a second, 2.9 GB of device memory) and merges
its section into the record:

    python scripts/bench_tb_targets.py kernel  [out.json]   gbl_tb_targets at 4 096 and 65 536 rows of the masked-random mix (seed 11,
                                                            64 plies: bench_tablebase.py's positions) on the full table, all outputs
                                                            but the dense outcome rows; beside it, alternating in the same process,
                                                            gbl_decode_obs + gbl_tb_probe + the torch operations that build visits, z
                                                            and the census-free targets from the probe's rows
    python scripts/bench_tb_targets.py guard   [out.json]   the two medians of tests/test_gpu_tb_targets_guard.py: 65 536 rows on the
                                                            (1, 1, 2) table of pseudo-random bytes, visits_out and z_out only,
                                                            against gbl_decode_obs + gbl_tb_probe
    python scripts/bench_tb_targets.py relabel [out.json]   the launch ReplayBuffer.relabel makes over the ring of one 65 536-board x
                                                            32-ply window of tree-against-tree self-play, and the method itself
                                                            (which first reads the ring's counter)
    python scripts/bench_tb_targets.py fit     [out.json]   one step of ReplayBuffer.fit at batch 1 024 with targets=None and with
                                                            the table
    python scripts/bench_tb_targets.py census  [out.json]   that ring's census: the share of rows whose search argmax lies outside R,
                                                            and the share whose game outcome is not the true sign
    python scripts/bench_tb_targets.py example [out.json]   the example at its defaults: both networks' agreement with the table

Default record: profiles/r23/tb_targets.json.  Recorded numbers, no gate (the guard test asserts its own ratio)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_solver as BS  # noqa: E402  (timed, merge)
import bench_training_batch as B  # noqa: E402  (the window, timed_pair, stats)
import gobblet_rl_amd as G  # noqa: E402
from gobblet_rl_amd import _native as nat  # noqa: E402

DEV = B.DEV
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r23", "tb_targets.json")
SLICE = 1 << 28


def full_table():
    tb = G.Tablebase((2, 2, 2), DEV)
    tb.build(slice_positions=SLICE)
    assert tb.complete
    return tb


def mix_rows(n):
    """n observation rows and masks of the masked-random mix (seed 11, 64 plies)."""
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=11)
    env.rollout(64)
    torch.cuda.synchronize()
    return env.observation.reshape(n, nat.OBS_BYTES).clone(), env.action_mask.clone()


def launchers(tb, obs, mask, dense):
    """Two callables on the same rows with preallocated outputs: the new kernel, and the two launches it folds (with `dense` also the
    torch operations that turn the probe's rows into visits and z)."""
    n, lib, s = obs.shape[0], nat.lib(), nat.current_stream(DEV)
    visits, z = torch.zeros((n, nat.ACTIONS), dtype=torch.int16, device=DEV), torch.zeros(n, dtype=torch.int8, device=DEV)
    value = torch.zeros(n, dtype=torch.int8, device=DEV)
    state, who = torch.empty((n, nat.CELLS), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)
    outcome, action = torch.empty((n, nat.ACTIONS), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    inv, aux, table = tb._inv, tb._aux.data_ptr(), tb.table.data_ptr()

    def targets():
        nat.check(lib.gbl_tb_targets(inv, aux, table, obs.data_ptr(), nat.OBS_BYTES, nat.ptr(mask), nat.ACTIONS, None, visits.data_ptr(), nat.ACTIONS,
                                     None, z.data_ptr(), 1, 0, 1, value.data_ptr() if dense else None, None, None, n, s), "gbl_tb_targets")

    def composition():
        nat.check(lib.gbl_decode_obs(obs.data_ptr(), state.data_ptr(), who.data_ptr(), n, s), "gbl_decode_obs")
        nat.check(lib.gbl_tb_probe(inv, aux, table, state.data_ptr(), who.data_ptr(), nat.ptr(mask), outcome.data_ptr(), value.data_ptr(),
                                   action.data_ptr(), n, s), "gbl_tb_probe")
        if dense:
            sign = torch.sign(value)
            keeps = (outcome != nat.SOLVE_NONE) & (torch.sign(outcome) == sign[:, None]) & (action >= 0)[:, None]
            visits.copy_(keeps)
            z.copy_(torch.where(action >= 0, sign, torch.full_like(sign, nat.Z_OPEN)))

    return targets, composition, (visits, z)


def kernel(path):
    tb = full_table()
    rows = []
    for n in (4096, 65536):
        obs, mask = mix_rows(n)
        targets, composition, (visits, z) = launchers(tb, obs, mask, dense=True)
        targets()
        mine = (visits.clone(), z.clone())
        composition()
        torch.cuda.synchronize()
        assert torch.equal(mine[0], visits) and torch.equal(mine[1], z), "the kernel and the composition disagree"
        t = B.timed_pair({"gbl_tb_targets": targets, "decode_obs + tb_probe + torch": composition})
        row = {"rows": n, **{k: B.stats(v) for k, v in t.items()}}
        print(json.dumps(row), flush=True)
        rows.append(row)
    BS.merge(path, "kernel", {"device": torch.cuda.get_device_name(0), "table": "(2, 2, 2), complete", "rows": rows})


def guard_pair(n=65536):
    """The guard's two callables: n rows of (1, 1, 2) positions, both movers, on pseudo-random bytes."""
    tb = G.Tablebase((1, 1, 2), DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    tb.table.copy_(torch.randint(-128, 128, (tb.positions,), dtype=torch.int8, device=DEV, generator=gen))
    st = tb.position(torch.randint(0, tb.positions, (n,), device=DEV, generator=gen))
    who = (torch.arange(n, device=DEV) % 2).to(torch.int8)
    st = torch.where(who[:, None] == 1, -st, st).contiguous()
    obs = torch.empty((n, nat.OBS_BYTES), dtype=torch.int8, device=DEV)
    nat.check(nat.lib().gbl_observe(st.data_ptr(), who.data_ptr(), -1, obs.data_ptr(), n, nat.current_stream(DEV)), "gbl_observe")
    targets, composition, _ = launchers(tb, obs, None, dense=False)
    return {"gbl_tb_targets": targets, "gbl_decode_obs + gbl_tb_probe": composition}


def guard(path):
    t = B.timed_pair(guard_pair())
    BS.merge(path, "guard", {"rows": 65536, "table": "(1, 1, 2), pseudo-random bytes", **{k: B.stats(v) for k, v in t.items()}})


def selfplay_ring():
    import bench_replay as P
    env, traj = B.window()
    return P.filled_buffer(env, traj)


def relabel(path):
    tb, buf = full_table(), selfplay_ring()
    live = buf.size

    def launch():
        tb._targets(live, buf._obs.data_ptr(), nat.REPLAY_OBS_PITCH, buf._meta.data_ptr(), nat.REPLAY_META_PITCH, buf._visits.data_ptr(),
                    nat.REPLAY_VISITS_PITCH, buf._meta.data_ptr() + nat.REPLAY_META_Z, nat.REPLAY_META_PITCH, "result", 1, False, None, False)

    t = B.timed_pair({"launch": launch, "ReplayBuffer.relabel": lambda: buf.relabel(tb)})
    BS.merge(path, "relabel", {"ring_rows": live, "ring_bytes": live * 320, **{k: B.stats(v) for k, v in t.items()}})


def fit(path):
    tb, buf = full_table(), selfplay_ring()
    a, b = G.GobbletTrainer(hidden=64, device=DEV, seed=0), G.GobbletTrainer(hidden=64, device=DEV, seed=0)
    t = B.timed_pair({"fit step, targets=None": lambda: buf.fit(a, 1, batch=1024), "fit step, targets=tb": lambda: buf.fit(b, 1, batch=1024, targets=tb)})
    BS.merge(path, "fit_step", {"batch": 1024, "hidden": 64, **{k: B.stats(v) for k, v in t.items()}})


def census(path):
    tb, buf = full_table(), selfplay_ring()
    c = buf.relabel(tb, census=True).cpu().numpy().astype(int)
    labelled = c >= 0
    searched = labelled & ((c & 4) == 0)
    rec = {"ring_rows": int(len(c)), "labelled_rows": int(labelled.sum()), "rows_with_search_visits": int(searched.sum()),
           "search_argmax_outside_R": int((searched & ((c & 1) == 0)).sum()), "game_outcome_is_not_the_true_sign": int((labelled & ((c & 2) == 0)).sum())}
    rec["share_argmax_outside_R"] = rec["search_argmax_outside_R"] / max(rec["rows_with_search_visits"], 1)
    rec["share_outcome_not_true_sign"] = rec["game_outcome_is_not_the_true_sign"] / max(rec["labelled_rows"], 1)
    print(json.dumps(rec), flush=True)
    BS.merge(path, "census_of_a_selfplay_ring", rec)


def example(path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import example_train_tablebase as ex
    rec = ex.train_both(DEV)
    print(json.dumps(rec), flush=True)
    BS.merge(path, "example_networks", rec)


if __name__ == "__main__":
    {"kernel": kernel, "guard": guard, "relabel": relabel, "fit": fit, "census": census, "example": example}[sys.argv[1]](
        sys.argv[2] if len(sys.argv) > 2 else DEFAULT_OUT)
