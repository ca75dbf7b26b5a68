#!/usr/bin/env python3
"""Records tests/golden/train_weighted_arg_errors.json: bad calls of gbl_train_step_weighted and gbl_replay_importance with the return
code and the last-error text of either flavour, as scripts/record_train_arg_errors.py does for gbl_train_step (no GPU needed: every
call returns before any device work; the pointers are numbers, never read).  A case whose "host" is null is an alignment rule, which
only the device flavour has.

    python scripts/record_train_weighted_arg_errors.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gobblet_rl_amd import _native as nat  # noqa: E402

K = 65536
FULL = 4 * 1024 * (2 * 64 + 60)  # gbl_train_workspace_bytes(1024, 64)
INF, NAN = float("inf"), float("nan")
STEP = dict(obs=1 * K, mask=2 * K, visits=3 * K, z=4 * K, batch=1024, hidden=64, params=5 * K, adam_m=6 * K, adam_v=7 * K, hyper=8 * K,
            row_weight=11 * K, row_loss_out=12 * K, prio_out=13 * K, prio_scale=1000.0, prio_floor=1, prio_cap=100000,
            grad_out=9 * K, stats_out=10 * K, workspace=16 * K, workspace_bytes=FULL, stream=None)
STEP_CASES = [
    ("hidden = 96", dict(hidden=96)), ("batch = 0", dict(batch=0)), ("batch = 65537", dict(batch=65537, workspace_bytes=1 << 40)),
    ("hidden before batch", dict(hidden=63, batch=0)),
    ("no obs", dict(obs=None)), ("no visits", dict(visits=None)), ("no z", dict(z=None)), ("no params", dict(params=None)),
    ("no adam_m", dict(adam_m=None)), ("no adam_v", dict(adam_v=None)), ("no hyper", dict(hyper=None)),
    ("no stats_out", dict(stats_out=None)), ("no workspace", dict(workspace=None)),
    ("workspace one byte short", dict(workspace_bytes=FULL - 1)),
    ("obs misaligned", dict(obs=1 * K + 8)), ("mask misaligned", dict(mask=2 * K + 1)), ("visits misaligned", dict(visits=3 * K + 2)),
    ("params misaligned", dict(params=5 * K + 4)), ("adam_m misaligned", dict(adam_m=6 * K + 8)),
    ("adam_v misaligned", dict(adam_v=7 * K + 12)), ("grad_out misaligned", dict(grad_out=9 * K + 4)),
    ("stats_out misaligned", dict(stats_out=10 * K + 4)), ("workspace misaligned", dict(workspace=16 * K + 8)),
    ("prio_scale < 0", dict(prio_scale=-1.0)), ("prio_scale = inf", dict(prio_scale=INF)), ("prio_scale = nan", dict(prio_scale=NAN)),
    ("prio_floor < 0", dict(prio_floor=-1)), ("prio_cap < prio_floor", dict(prio_floor=5, prio_cap=4)),
    ("prio_scale before prio_floor", dict(prio_scale=-1.0, prio_floor=-1)),
    ("a missing pointer before prio_scale", dict(prio_scale=-1.0, z=None)),
    ("gbl_train_step's alignment before prio_scale", dict(prio_scale=-1.0, params=5 * K + 4)),
    ("row_weight misaligned", dict(row_weight=11 * K + 2)), ("row_loss_out misaligned", dict(row_loss_out=12 * K + 1)),
    ("prio_out misaligned", dict(prio_out=13 * K + 3)),
    ("prio_floor before the new arrays' alignment", dict(prio_floor=-1, row_weight=11 * K + 2)),
]
IMP = dict(prio=1 * K, batch=1024, beta=0.5, weights_out=2 * K, stream=None)
IMP_CASES = [
    ("batch = 0", dict(batch=0)), ("batch < 0", dict(batch=-3)), ("batch = 65537", dict(batch=65537)),
    ("beta < 0", dict(beta=-0.25)), ("beta > 1", dict(beta=1.5)), ("beta = nan", dict(beta=NAN)),
    ("batch before beta", dict(batch=0, beta=2.0)),
    ("no prio", dict(prio=None)), ("no weights_out", dict(weights_out=None)), ("beta before the pointers", dict(beta=2.0, prio=None)),
    ("prio misaligned", dict(prio=1 * K + 2)), ("weights_out misaligned", dict(weights_out=2 * K + 1)),
    ("a missing pointer before an alignment error", dict(prio=None, weights_out=2 * K + 1)),
]


def main():
    dev, host = nat.lib(), nat.cpu_raw()
    table = []
    for fn, base, cases in (("train_step_weighted", STEP, STEP_CASES), ("replay_importance", IMP, IMP_CASES)):
        for name, kw in cases:
            args = [dict(base, **kw)[k] for k in base]
            rc = getattr(dev, "gbl_" + fn)(*args)
            assert rc != 0, (fn, name)  # (a good call would launch)
            row = {"fn": fn, "case": name, "args": args, "device": [rc, dev.gbl_last_error().decode()], "host": None}
            if rc != nat.ERR_ALIGN:
                rc = getattr(host, "gbl_cpu_" + fn)(*args)
                assert rc != 0, (fn, name)
                row["host"] = [rc, host.gbl_cpu_last_error().decode()]
            table.append(row)
    with open(os.path.join(ROOT, "tests", "golden", "train_weighted_arg_errors.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in table) + "\n]\n")
    print(len(table), "cases")


if __name__ == "__main__":
    main()
