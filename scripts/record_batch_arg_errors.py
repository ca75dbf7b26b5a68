#!/usr/bin/env python3
"""Records tests/golden/batch_arg_errors.json: bad calls of gbl_symmetry_apply and gbl_training_batch (every single violation, double
ones that pin which check fires first, and the n == 0 / batch == 0 returns) with the return code and message of either flavour.
Every call returns before any device work -- the pointers are numbers that are never read -- so it runs without a GPU:
    python scripts/record_batch_arg_errors.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gobblet_rl_amd import _native as nat  # noqa: E402

P = [0x10000 * (i + 1) for i in range(16)]  # sixteen distinct 16-byte aligned "pointers"

# gbl_symmetry_apply(sym, sym_all, agent, state_in, state_out, obs_in, obs_out, mask_in, mask_out, visits_in, visits_out, priors_in,
#                    priors_out, actions_in, actions_out, n, stream)
APPLY = dict(sym=P[0], sym_all=0, agent=P[1], state_in=P[2], state_out=P[3], obs_in=P[4], obs_out=P[5], mask_in=P[6], mask_out=P[7],
             visits_in=P[8], visits_out=P[9], priors_in=P[10], priors_out=P[11], actions_in=P[12], actions_out=P[13], n=100, stream=None)
# gbl_training_batch(obs_traj, mask_traj, visits_traj, z_traj, done_traj, mover_traj, n, plies, ply_stride, tile_stride, batch, sym_mask,
#                    seed, sample_base, call, obs_out, mask_out, visits_out, z_out, index_out, sym_out, stream)
BATCH = dict(obs_traj=P[0], mask_traj=P[1], visits_traj=P[2], z_traj=P[3], done_traj=P[4], mover_traj=P[5], n=200, plies=12, ply_stride=256,
             tile_stride=64, batch=1000, sym_mask=511, seed=1, sample_base=0, call=0, obs_out=P[6], mask_out=P[7], visits_out=P[8], z_out=P[9],
             index_out=P[10], sym_out=P[11], stream=None)

CASES = [("symmetry_apply", APPLY, name, ch) for name, ch in [
    ("n < 0", dict(n=-1)),
    ("n < 0 before sym_all", dict(n=-1, sym=None, sym_all=512)),
    ("sym_all = 512", dict(sym=None, sym_all=512)),
    ("sym_all = -1", dict(sym=None, sym_all=-1)),
    ("sym_all out of range before n == 0", dict(sym=None, sym_all=600, n=0)),
    ("sym_all ignored when sym is given: n == 0 returns OK", dict(sym_all=600, n=0)),
    ("n == 0 returns OK whatever the pointers", dict(n=0, state_out=None, agent=None)),
    ("state_in without state_out", dict(state_out=None)),
    ("state_out without state_in", dict(state_in=None)),
    ("obs_in without obs_out", dict(obs_out=None)),
    ("mask_out without mask_in", dict(mask_in=None)),
    ("visits_in without visits_out", dict(visits_out=None)),
    ("priors_out without priors_in", dict(priors_in=None)),
    ("actions_in without actions_out", dict(actions_out=None)),
    ("state in place", dict(state_out=P[2])),
    ("obs in place", dict(obs_out=P[4])),
    ("mask in place", dict(mask_out=P[6])),
    ("visits in place", dict(visits_out=P[8])),
    ("priors in place", dict(priors_out=P[10])),
    ("actions in place", dict(actions_out=P[12])),
    ("the pair check of an earlier row fires first", dict(state_out=None, obs_out=P[4])),
    ("no agent with obs", dict(agent=None)),
    ("no agent with actions alone", dict(agent=None, state_in=None, state_out=None, obs_in=None, obs_out=None, mask_in=None, mask_out=None,
                                         visits_in=None, visits_out=None, priors_in=None, priors_out=None)),
    ("in place before the missing agent", dict(agent=None, mask_out=P[6])),
    ("state_in misaligned", dict(state_in=P[2] + 8)),
    ("obs_out misaligned", dict(obs_out=P[5] + 4)),
    ("mask_in misaligned", dict(mask_in=P[6] + 1)),
    ("visits_out misaligned", dict(visits_out=P[9] + 2)),
    ("priors_in misaligned", dict(priors_in=P[10] + 8)),
    ("actions_out misaligned", dict(actions_out=P[13] + 2)),
    ("sym misaligned", dict(sym=P[0] + 1)),
    ("an argument error before an alignment error", dict(state_in=P[2] + 8, n=-1)),
]] + [("training_batch", BATCH, name, ch) for name, ch in [
    ("plies = 1", dict(plies=1)),
    ("plies = 0", dict(plies=0)),
    ("plies = 32768", dict(plies=32768)),
    ("batch < 0", dict(batch=-1)),
    ("batch = 2^31 + 1", dict(batch=(1 << 31) + 1)),
    ("plies before batch", dict(plies=1, batch=-1)),
    ("sym_mask = 512", dict(sym_mask=512)),
    ("sym_mask = -1", dict(sym_mask=-1)),
    ("call = 2^26", dict(call=1 << 26)),
    ("batch == 0 returns OK whatever the pointers", dict(batch=0, n=0, visits_traj=None, index_out=None, ply_stride=3)),
    ("the scalar checks come before batch == 0", dict(batch=0, call=1 << 26)),
    ("n = 0", dict(n=0)),
    ("n < 0", dict(n=-5)),
    ("n = 2^31 + 1", dict(n=(1 << 31) + 1, ply_stride=1 << 40)),
    ("no visits_traj", dict(visits_traj=None)),
    ("no z_traj", dict(z_traj=None)),
    ("no done_traj", dict(done_traj=None)),
    ("no mover_traj", dict(mover_traj=None)),
    ("no index_out", dict(index_out=None)),
    ("obs_out without obs_traj", dict(obs_traj=None)),
    ("mask_out without mask_traj", dict(mask_traj=None)),
    ("n before the pointers", dict(n=0, z_traj=None)),
    ("ply_stride not a multiple of 16", dict(ply_stride=250)),
    ("ply_stride too small for the tiles (time-major)", dict(ply_stride=192)),
    ("tile_stride = 0", dict(tile_stride=0)),
    ("tile-major strides that overlap", dict(ply_stride=64, tile_stride=64 * 11)),
    ("the pointers before the strides", dict(ply_stride=250, done_traj=None)),
    ("obs_out misaligned", dict(obs_out=P[6] + 8)),
    ("mask_out misaligned", dict(mask_out=P[7] + 4)),
    ("visits_out misaligned", dict(visits_out=P[8] + 2)),
    ("visits_traj misaligned", dict(visits_traj=P[2] + 2)),
    ("index_out misaligned", dict(index_out=P[10] + 2)),
    ("sym_out misaligned", dict(sym_out=P[11] + 1)),
    ("the strides before an alignment error", dict(ply_stride=250, obs_out=P[6] + 8)),
]]


def main():
    dev, host = nat.lib(), nat.cpu_raw()
    table = []
    for fn, base, case, change in CASES:
        args = list({**base, **change}.values())
        row = {"fn": fn, "case": case, "args": args}
        merged = {**base, **change}
        rc = getattr(dev, "gbl_" + fn)(*args)  # the device flavour first: it alone knows the alignment rules
        row["device"] = [rc, dev.gbl_last_error().decode() if rc else ""]
        assert rc in (nat.ERR_ARG, nat.ERR_ALIGN) or (rc == 0 and (merged["n"] == 0 or merged.get("batch") == 0)), row
        if rc == nat.ERR_ALIGN:
            row["host"] = None  # (the host flavour has no alignment rules: such a call would go on to read the "pointers")
        else:
            rc = getattr(host, "gbl_cpu_" + fn)(*args)
            row["host"] = [rc, host.gbl_cpu_last_error().decode() if rc else ""]
            assert row["device"] == row["host"], row
        table.append(row)
    with open(os.path.join(ROOT, "tests", "golden", "batch_arg_errors.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in table) + "\n]\n")
    print(len(table), "cases")


if __name__ == "__main__":
    main()
