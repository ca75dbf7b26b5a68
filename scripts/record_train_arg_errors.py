#!/usr/bin/env python3
"""Records tests/golden/train_arg_errors.json: bad calls of gbl_train_step with the return code and the last-error text of either
flavour (no GPU needed: every call returns before any device work; the pointers are numbers, never read).  A case whose "host" is
null is an alignment rule, which only the device flavour has.

    python scripts/record_train_arg_errors.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gobblet_rl_amd import _native as nat  # noqa: E402

K = 65536
FULL = 4 * 1024 * (2 * 64 + 60)  # gbl_train_workspace_bytes(1024, 64)
BASE = dict(obs=1 * K, mask=2 * K, visits=3 * K, z=4 * K, batch=1024, hidden=64, params=5 * K, adam_m=6 * K, adam_v=7 * K, hyper=8 * K,
            grad_out=9 * K, stats_out=10 * K, workspace=16 * K, workspace_bytes=FULL, stream=None)
CASES = [
    ("hidden = 0", dict(hidden=0)), ("hidden = 96", dict(hidden=96)), ("hidden = 320", dict(hidden=320)),
    ("batch = 0", dict(batch=0)), ("batch < 0", dict(batch=-1)), ("batch = 65537", dict(batch=65537, workspace_bytes=1 << 40)),
    ("hidden before batch", dict(hidden=63, batch=0)),
    ("no obs", dict(obs=None)), ("no visits", dict(visits=None)), ("no z", dict(z=None)), ("no params", dict(params=None)),
    ("no adam_m", dict(adam_m=None)), ("no adam_v", dict(adam_v=None)), ("no hyper", dict(hyper=None)),
    ("no stats_out", dict(stats_out=None)), ("no workspace", dict(workspace=None)),
    ("batch before the pointers", dict(batch=0, obs=None)),
    ("workspace one byte short", dict(workspace_bytes=FULL - 1)), ("workspace_bytes = 0", dict(workspace_bytes=0)),
    ("workspace_bytes < 0", dict(workspace_bytes=-5)), ("workspace of H = 64 given to H = 256", dict(hidden=256)),
    ("the pointers before the workspace size", dict(workspace_bytes=0, z=None)),
    ("obs misaligned", dict(obs=1 * K + 8)), ("mask misaligned", dict(mask=2 * K + 1)), ("visits misaligned", dict(visits=3 * K + 2)),
    ("params misaligned", dict(params=5 * K + 4)), ("adam_m misaligned", dict(adam_m=6 * K + 8)),
    ("adam_v misaligned", dict(adam_v=7 * K + 12)), ("grad_out misaligned", dict(grad_out=9 * K + 4)),
    ("stats_out misaligned", dict(stats_out=10 * K + 4)), ("workspace misaligned", dict(workspace=16 * K + 8)),
    ("an argument error before an alignment error", dict(obs=1 * K + 8, workspace_bytes=0)),
]


def main():
    dev, host = nat.lib(), nat.cpu_raw()
    table = []
    for name, kw in CASES:
        args = [dict(BASE, **kw)[k] for k in BASE]
        rc = dev.gbl_train_step(*args)
        assert rc != 0, name  # (a good call would launch)
        row = {"fn": "train_step", "case": name, "args": args, "device": [rc, dev.gbl_last_error().decode()], "host": None}
        if rc != nat.ERR_ALIGN:
            rc = host.gbl_cpu_train_step(*args)
            row["host"] = [rc, host.gbl_cpu_last_error().decode()]
        table.append(row)
    with open(os.path.join(ROOT, "tests", "golden", "train_arg_errors.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in table) + "\n]\n")
    print(len(table), "cases")


if __name__ == "__main__":
    main()
