#!/usr/bin/env python3
"""Records tests/golden/selfplay_arg_errors.json: the argument checks of the four self-play entry points (gbl_collect_search, _eval,
_solve, _noise) IN THEIR ORDER, with the return code and the last-error text of either flavour.  Per function: every check alone,
every adjacent pair of checks broken together (the earlier one answers), a clean call, and the n == 0 / plies == 0 early returns
in front of arguments a later check would refuse.  No GPU needed: every call returns before any work; the pointers are numbers,
never read (so no case here may pass every check with n > 0 and plies > 0).  A case whose "host" is null is an alignment rule,
which only the device flavour has.  Every "ev" of an argument list is the next entry of "evs": eight fields, or null.

    python scripts/record_selfplay_arg_errors.py"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gobblet_rl_amd import _native as nat  # noqa: E402

K = 65536
GOOD_EV = [1 * K, 2 * K, 3 * K, 4 * K, 64, 4, 9, 9]


def short(name):
    """The ABI's parameter name as base() and the cases spell it: a trajectory array without its "_traj" (but done_traj / to_move_traj)."""
    return name[:-5] if name.endswith("_traj") and name[:-5] not in ("done", "to_move") else name


def names(fn):
    """The arguments of gbl_`fn` in the ABI's order (nat.SELFPLAY_ARGS)."""
    return tuple(short(k) for k, _ in nat.SELFPLAY_ARGS["gbl_" + fn])


def traj_of(fn):
    return tuple(short(k) for k, _ in nat.SELFPLAY_ARGS["gbl_" + fn] if k.endswith("_traj"))


def base(fn):
    """Arguments that pass every check (and so must never be called as they are: n and plies are positive)."""
    code = nat.POLICY_TREE if fn == "collect_search" else nat.POLICY_EVAL_TREE
    b = dict(state=5 * K, to_move=6 * K, done=7 * K, n=5, ply_stride=128, tile_stride=64, seed=1, env_base=0, ply0=0, ply_dev=None,
             plies=2, policy0=code, policy1=code, iterations0=8, iterations1=8, playouts0=2, playouts1=2, max_plies=8, explore=16,
             ev0=GOOD_EV, ev1=GOOD_EV, solve_depth0=2, solve_depth1=0, noise0=64, noise1=64, sample_plies=0, illegal_mode=0,
             counters=None, turn=None, stream=None)
    b.update({k: (8 + i) * K for i, k in enumerate(traj_of(fn))})
    return {k: b[k] for k in names(fn)}


def ev(**kw):
    e = list(GOOD_EV)
    for k, v in kw.items():
        e[("w1", "b1", "w2", "b2", "hidden", "shift1", "shift_p", "shift_v").index(k)] = v
    return e


def checks(fn):
    """[(name, overrides)] in the order the entry point looks at them; each breaks exactly one rule."""
    evaluator = fn != "collect_search"
    c = [("n < 0", dict(n=-1)), ("illegal_mode", dict(illegal_mode=2)), ("policy0", dict(policy0=nat.POLICY_GREEDY1))]
    if evaluator:
        c += [("ev0 NULL", dict(ev0=None)), ("ev0 hidden", dict(ev0=ev(hidden=96))), ("ev0 shift", dict(ev0=ev(shift_p=25))),
              ("iterations0", dict(iterations0=513)), ("explore", dict(explore=1025)), ("ev1 NULL", dict(ev1=None)),
              ("iterations1", dict(iterations1=0))]
    else:
        c += [("iterations0", dict(iterations0=1025)), ("playouts0", dict(playouts0=0)), ("iterations1", dict(iterations1=0)),
              ("playouts1", dict(playouts1=257)), ("max_plies", dict(max_plies=256)), ("explore", dict(explore=-1))]
    c += [("sample_plies < 0", dict(sample_plies=-1)), ("sample_plies without turn", dict(sample_plies=2)),
          ("ply0 + plies", dict(ply0=(1 << 24) - 1)), ("env_base + n", dict(env_base=(1 << 42) - 4))]
    if fn in ("collect_search_solve", "collect_search_noise"):
        c += [("solve_depth0", dict(solve_depth0=7)), ("solve_depth1", dict(solve_depth1=-1))]
    if fn == "collect_search_noise":
        c += [("noise0", dict(noise0=-1)), ("noise1", dict(noise1=257))]
    c += [("state NULL", dict(state=None)), ("to_move NULL", dict(to_move=None)), ("done NULL", dict(done=None))]
    if evaluator:
        c += [("ev0 w1 NULL", dict(ev0=ev(w1=None))), ("ev0 b2 misaligned", dict(ev0=ev(b2=4 * K + 8))),
              ("ev1 w2 NULL", dict(ev1=ev(w2=None))), ("ev1 w1 misaligned", dict(ev1=ev(w1=1 * K + 4)))]
    c += [("strides", dict(ply_stride=8)), ("state misaligned", dict(state=5 * K + 4)), ("mask_traj misaligned", dict(mask=13 * K + 8)),
          ("obs_traj misaligned", dict(obs=14 * K + 8)), ("reward_traj misaligned", dict(reward=10 * K + 1)),
          ("actions_traj misaligned", dict(actions=8 * K + 2))]
    if evaluator:
        c += [("root_value_traj misaligned", dict(root_value=20 * K + 2))]
    c += [("turn misaligned", dict(turn=30 * K + 2)), ("counters misaligned", dict(counters=31 * K + 64)),
          ("visits_traj misaligned", dict(visits=15 * K + 1))]
    return c


def cases(fn):
    c = checks(fn)
    out = list(c)
    for (a, ka), (b, kb) in zip(c, c[1:]):
        if not set(ka) & set(kb):  # (two rules on one argument cannot be broken together)
            out.append(("%s before %s" % (a, b), dict(ka, **kb)))
    late = dict(ply_stride=8, actions=8 * K + 2, visits=15 * K + 1)  # what the checks after both early returns refuse
    out += [("clean, n = 0", dict(n=0)), ("n = 0 before the pointers and the strides", dict(n=0, state=None, done=None, **late)),
            ("the window before n = 0", dict(n=0, ply0=1 << 24)), ("plies = 0 before the strides and the alignments", dict(plies=0, **late)),
            ("the pointers before plies = 0", dict(plies=0, to_move=None)), ("the window before plies = 0", dict(plies=0, illegal_mode=-1))]
    if fn != "collect_search":
        out += [("n = 0 before the evaluator's pointers", dict(n=0, ev0=ev(w1=None), ev1=ev(b1=2 * K + 4))),
                ("plies = 0 before the evaluator's pointers", dict(plies=0, ev0=ev(w1=None), ev1=ev(b1=2 * K + 4))),
                ("a RANDOM side's evaluator, budget and pointers are not read",
                 dict(n=0, policy1=nat.POLICY_RANDOM, ev1=None, iterations1=0, solve_depth1=99, noise1=999)),
                ("an evaluator's pointers before their alignment", dict(ev0=ev(w1=None, b2=4 * K + 8))),
                ("the evaluator's pointers before the strides", dict(ev1=ev(w2=None), ply_stride=8))]
    if fn == "collect_search_noise":
        out += [("the weight before n = 0", dict(n=0, noise1=300)), ("the weight before the pointers", dict(noise0=257, state=None))]
    return [(name, {k: v for k, v in kw.items() if k in names(fn)}) for name, kw in out]


def call(lib, prefix, fn, args, evs):
    """One call as the table records it (tests/search_harness.py's recorded_call replays it): "ev" is the next evaluator of `evs`."""
    structs = [None if e is None else nat.Evaluator(*e) for e in evs]
    it = iter(structs)
    real = []
    for x in args:
        if x == "ev":
            e = next(it)
            x = None if e is None else C.addressof(e)
        real.append(x)
    rc = getattr(lib, prefix + fn)(*real)
    return [rc, getattr(lib, prefix + "last_error")().decode() if rc else ""]


def main():
    dev, host = nat.lib(), nat.cpu_raw()
    table = []
    for fn in ("collect_search", "collect_search_eval", "collect_search_solve", "collect_search_noise"):
        for name, kw in cases(fn):
            a = dict(base(fn), **kw)
            assert a["n"] <= 0 or a["plies"] == 0 or kw, (fn, name)
            evs = [a[k] for k in ("ev0", "ev1") if k in a]
            args = ["ev" if k in ("ev0", "ev1") else a[k] for k in names(fn)]
            row = {"fn": fn, "case": name, "args": args, "evs": evs, "device": call(dev, "gbl_", fn, args, evs), "host": None}
            assert row["device"][0] != nat.ERR_HIP and (row["device"][0] != 0 or a["n"] == 0 or a["plies"] == 0), (fn, name)  # (a good call would launch)
            if row["device"][0] != nat.ERR_ALIGN:
                row["host"] = call(host, "gbl_cpu_", fn, args, evs)
            table.append(row)
    with open(os.path.join(ROOT, "tests", "golden", "selfplay_arg_errors.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in table) + "\n]\n")
    print(len(table), "cases")


if __name__ == "__main__":
    main()
