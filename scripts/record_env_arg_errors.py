#!/usr/bin/env python3
"""Records tests/golden/env_arg_errors.json: the argument checks of the env, collect and greedy entry points (gbl_reset ... gbl_board_eval,
gbl_step*, gbl_sample*, gbl_rollout*, gbl_collect*, gbl_collect_policy, gbl_decode_obs, gbl_validate, gbl_greedy*) IN THEIR ORDER, with the
return code and the last-error text of either flavour, in the format and by the rules of scripts/record_selfplay_arg_errors.py.  Per
function: every check alone, every adjacent pair of checks broken together (the table says which one answers), and the n == 0 /
plies == 0 early returns in front of arguments a later check would refuse.  No GPU needed: every call returns before any work; the
pointers are numbers, never read (so no case here may pass every check with n > 0 and plies > 0).  "host" is null where only the device
flavour can answer: a case that breaks nothing but alignment rules, and every case of the helpers without a host flavour
(gbl_collect_variant, gbl_pinned_alloc, gbl_block_alloc, gbl_placement_probe).  Where a case breaks an alignment rule AND another, each
flavour's answer is recorded as it is (gbl_collect_from_ex looks at first_actions' alignment before its NULL checks).

    python scripts/record_env_arg_errors.py"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gobblet_rl_amd import _native as nat  # noqa: E402

K = 65536
_STEP = "state to_move done actions winner_out reward_out mask_out obs_out turn"
_ROLL = "state to_move done actions_out winner_out reward_out mask_out obs_out n seed env_base ply0"
_TRAJ = "actions_traj winner_traj reward_traj done_traj to_move_traj mask_traj obs_traj"
_WINDOW = "n ply_stride tile_stride seed env_base ply0 ply_dev plies"
_GREEDY = "action_out chosen_out cand_mask_out fallback_out n stream"
# the arguments of gbl_<fn>, in the ABI's order (include/gobblet_hip.h)
SIGS = {fn: sig.split() for fn, sig in {
    "layout_info": "out",
    "reset": "state to_move done winner n stream",
    "legal_mask": "state to_move mask n stream",
    "is_legal": "state agent_index actions out n stream",
    "play_turn": "state agent_index actions n stream",
    "winner": "state winner n stream",
    "flatboard": "state flat n stream",
    "covered": "state cov n stream",
    "validate": "state flags n stream",
    "observe": "state to_move agent_sel obs n stream",
    "board_eval": "state agent_index actions record_out n stream",
    "step": _STEP + " n illegal_mode auto_reset stream",
    "step_into": _STEP + " actions_out done_out to_move_out n illegal_mode auto_reset stream",
    "step_ex": _STEP + " actions_out done_out to_move_out status_out next_actions_out seed env_base ply ply_dev n illegal_mode auto_reset stream",
    "sample": "mask actions n seed env_base ply stream",
    "sample_at": "mask actions n seed env_base ply ply_dev stream",
    "counter_add": "counter by stream",
    "rollout": _ROLL + " plies illegal_mode counters turn stream",
    "rollout_at": _ROLL + " ply_dev plies illegal_mode counters turn stream",
    "collect": "state to_move done " + _TRAJ + " " + _WINDOW + " illegal_mode counters turn stream",
    "collect_from": "state to_move done first_actions " + _TRAJ + " " + _WINDOW + " illegal_mode counters turn stream",
    "collect_from_ex": "state to_move done first_actions first_status " + _TRAJ + " " + _WINDOW + " illegal_mode counters turn stream",
    "collect_policy": "state to_move done hist " + _TRAJ + " chosen_traj how_traj cand_traj " + _WINDOW +
                      " policy0 policy1 opening_plies illegal_mode counters turn stream",
    "decode_obs": "obs state to_move n stream",
    "greedy": "state to_move mask hist depth action_out cand_mask_out fallback_out n stream",
    "greedy_act": "state to_move mask hist depth seed env_base call " + _GREEDY,
    "greedy_act_at": "state to_move mask hist depth seed env_base call call_dev " + _GREEDY,
    "collect_variant": "n plies with_mask with_obs",
    "pinned_alloc": "bytes host_ptr dev_ptr",
    "block_alloc": "bytes dev_ptr",
    "placement_probe": "a a_bytes b b_bytes slot_boards plies us_both us_a us_b stream",
}.items()}
NO_HOST = ("collect_variant", "pinned_alloc", "block_alloc", "placement_probe")
SCALARS = dict(n=5, stream=None, agent_sel=-1, illegal_mode=0, auto_reset=1, seed=1, env_base=0, ply=0, ply0=0, plies=2, by=1,
               ply_stride=128, tile_stride=64, policy0=nat.POLICY_GREEDY2, policy1=nat.POLICY_RANDOM, opening_plies=0, depth=2, call=0,
               with_mask=1, with_obs=1, bytes=4096, a_bytes=1 << 20, b_bytes=1 << 20, slot_boards=0)
# (optional arguments that start out NULL: a case sets the ones it is about)
ABSENT = ("ply_dev", "call_dev", "counters", "turn", "first_actions", "first_status")


def base(fn):
    """Arguments that pass every check (and so must never be called as they are): every pointer its own multiple of 64 KiB."""
    return {k: SCALARS[k] if k in SCALARS else None if k in ABSENT else (3 + i) * K for i, k in enumerate(SIGS[fn])}


def null(*names):
    return [("%s NULL" % k, dict([(k, None)]), "arg") for k in names]


def off(fn, by, *names):
    """`names` each moved `by` bytes off its place in base(fn): an alignment rule of the device flavour."""
    at = {k: (3 + i) * K for i, k in enumerate(SIGS[fn])}
    return [("%s misaligned" % k, dict([(k, at[k] + by)]), "align") for k in names]


N, MODE = [("n < 0", dict(n=-1), "arg")], [("illegal_mode", dict(illegal_mode=2), "arg")]


def checks(fn):
    """[(name, overrides, "arg" or "align")] in the order the entry point looks at them; each breaks exactly one rule."""
    def o(by, *names):
        return off(fn, by, *names)
    if fn in ("layout_info", "counter_add"):
        return null(SIGS[fn][0])
    if fn == "reset":
        return N + null("state", "to_move", "done")
    if fn == "legal_mask":
        return N + null("state", "to_move", "mask") + o(8, "state", "mask")
    if fn in ("is_legal", "play_turn", "winner", "validate"):
        return N + null(*SIGS[fn][:-2]) + o(8, "state")
    if fn in ("flatboard", "covered"):
        return N + null(*SIGS[fn][:2]) + o(8, *SIGS[fn][:2])
    if fn == "observe":
        return N + null("state", "obs") + [("agent_sel", dict(agent_sel=2), "arg"), ("agent_sel low", dict(agent_sel=-2), "arg")] + \
            null("to_move") + o(8, "state", "obs")
    if fn == "board_eval":
        return N + null("state", "record_out", "agent_index") + o(8, "state", "record_out") + o(2, "actions")
    if fn in ("step", "step_into", "step_ex"):
        words = [k for k in ("actions_out", "next_actions_out") if k in SIGS[fn]]
        return N + null("state", "to_move", "done", "actions") + MODE + o(8, "state", "mask_out", "obs_out") + o(1, "reward_out") + \
            o(2, "turn", "actions", *words)
    if fn in ("sample", "sample_at"):
        return N + null("mask", "actions") + o(8, "mask")
    if fn in ("rollout", "rollout_at"):
        return N + null("state", "to_move", "done") + MODE + o(8, "state", "mask_out", "obs_out") + o(1, "reward_out") + \
            [("counters misaligned", dict(counters=40 * K + 64), "align"), ("turn misaligned", dict(turn=41 * K + 2), "align")] + \
            o(2, "actions_out")
    if fn in ("collect", "collect_from", "collect_from_ex", "collect_policy"):
        c = list(N)
        if "first_actions" in SIGS[fn]:
            c += [("first_actions misaligned", dict(first_actions=42 * K + 2), "align")]
        if "first_status" in SIGS[fn]:
            c += [("first_status without first_actions", dict(first_status=43 * K, first_actions=None), "arg")]
        c += null("state", "to_move", "done") + MODE
        if fn == "collect_policy":
            c += [("policy0", dict(policy0=-1), "arg"), ("policy1", dict(policy1=nat.POLICY_GREEDY3 + 1), "arg"),
                  ("opening_plies < 0", dict(opening_plies=-1), "arg"), ("opening_plies without turn", dict(opening_plies=2), "arg")]
        c += [("strides", dict(ply_stride=8), "arg")] + o(8, "state", "mask_traj", "obs_traj") + o(1, "reward_traj") + o(2, "actions_traj")
        if fn == "collect_policy":
            c += o(2, "chosen_traj")
        c += [("turn misaligned", dict(turn=41 * K + 2), "align"), ("counters misaligned", dict(counters=40 * K + 64), "align")]
        if fn == "collect_policy":
            c += o(8, "cand_traj") + o(1, "hist")
        return c
    if fn == "decode_obs":
        return N + null("obs", "state", "to_move") + o(8, "obs", "state")
    if fn in ("greedy", "greedy_act", "greedy_act_at"):
        need = ("state", "to_move", "action_out") if fn == "greedy" else ("state", "to_move", "hist", "action_out")
        return N + null(*need) + [("depth", dict(depth=0), "arg"), ("depth high", dict(depth=4), "arg")] + \
            o(8, "state", "mask", "cand_mask_out") + o(1, "hist")
    if fn == "collect_variant":
        return N
    if fn == "pinned_alloc":
        return [("bytes", dict(bytes=0), "arg")] + null("host_ptr", "dev_ptr")
    if fn == "block_alloc":
        return [("bytes", dict(bytes=-1), "arg")] + null("dev_ptr")
    if fn == "placement_probe":
        return null("a", "b", "us_both", "us_a", "us_b") + o(64, "a", "b") + \
            [("slot_boards off a pair of tiles", dict(slot_boards=192), "arg"), ("plies < 1", dict(slot_boards=128, plies=0), "arg"),
             ("a smaller than its rows", dict(slot_boards=128, a_bytes=128 * 2 * nat.OBS_BYTES - 1), "arg"),
             ("b smaller than its rows", dict(slot_boards=128, b_bytes=128 * 2 * nat.ACTIONS - 1), "arg"),
             ("too small", dict(a_bytes=4 * 64 * nat.OBS_BYTES * 2 - 1), "arg"),
             ("too large", dict(slot_boards=1 << 37, plies=1, a_bytes=1 << 62, b_bytes=1 << 62), "arg")]
    raise KeyError(fn)


def cases(fn):
    """[(name, overrides, whether only the device flavour can answer)]"""
    c = checks(fn)
    out = [(name, kw, kind == "align") for name, kw, kind in c]
    for (a, ka, kind_a), (b, kb, kind_b) in zip(c, c[1:]):
        if not set(ka) & set(kb):  # (two rules on one argument cannot be broken together)
            out.append(("%s with %s" % (a, b), dict(ka, **kb), kind_a == kind_b == "align"))
    sig = SIGS[fn]
    if "n" in sig and fn != "collect_variant":
        late = {k: v for _, kw, kind in c[1:] for k, v in kw.items() if k not in ("n", "plies")}  # (what every later check refuses, at once)
        late.update({k: None for k in ("state", "mask", "obs") if k in sig})
        out += [("clean, n = 0", dict(n=0), False), ("n = 0 before everything else", dict(late, n=0), False)]
    if "plies" in sig and fn != "collect_variant" and fn != "placement_probe":
        late = {k: v for _, kw, kind in c for k, v in kw.items() if kind == "align" and k != "first_actions"}
        if "ply_stride" in sig:
            late["ply_stride"] = 8
        out += [("clean, plies = 0", dict(plies=0), False), ("plies = 0 before the strides and the alignments", dict(late, plies=0), False),
                ("the pointers before plies = 0", dict(plies=0, to_move=None), False),
                ("illegal_mode before plies = 0", dict(plies=0, illegal_mode=-1), False)]
        if "first_actions" in sig:
            out += [("first_actions' alignment before plies = 0", dict(plies=0, first_actions=42 * K + 2), True)]
        if fn == "collect_policy":
            out += [("the policies before plies = 0", dict(plies=0, policy1=9), False),
                    ("the opening before plies = 0", dict(plies=0, opening_plies=1), False)]
    if fn == "observe":
        out += [("a fixed agent_sel needs no to_move", dict(agent_sel=1, to_move=None, state=3 * K + 8), True)]
    if fn == "board_eval":
        out += [("without actions agent_index may be NULL", dict(actions=None, agent_index=None, state=3 * K + 8), True)]
    if fn == "collect_from_ex":
        out += [("first_status with first_actions", dict(first_actions=42 * K, first_status=43 * K, done=None), False),
                ("first_actions' alignment before the pointers", dict(first_actions=42 * K + 2, state=None), False)]
    return out


def call(lib, prefix, fn, args):
    """One call as the table records it (tests/search_harness.py's recorded_call replays it): a number where the ABI has a typed
    pointer is cast to it."""
    f = getattr(lib, prefix + fn)
    assert len(args) == len(f.argtypes), fn
    real = [C.cast(x, t) if isinstance(x, int) and isinstance(t, type) and issubclass(t, C._Pointer) else x for x, t in zip(args, f.argtypes)]
    rc = f(*real)
    return [rc, getattr(lib, prefix + "last_error")().decode() if rc else ""]


def main():
    dev, host = nat.lib(), nat.cpu_raw()
    table = []
    for fn in SIGS:
        for name, kw, device_only in cases(fn):
            assert kw and set(kw) <= set(SIGS[fn]), (fn, name)
            a = dict(base(fn), **kw)
            args = [a[k] for k in SIGS[fn]]
            row = {"fn": fn, "case": name, "args": args, "device": call(dev, "gbl_", fn, args), "host": None}
            early = a.get("n", 1) == 0 or ("plies" in a and a["plies"] == 0)
            assert row["device"][0] != nat.ERR_HIP and (row["device"][0] < 0 or early), (fn, name, row)  # (a good call would launch)
            assert not device_only or row["device"][0] == nat.ERR_ALIGN, (fn, name, row)
            if fn not in NO_HOST and not device_only:
                row["host"] = call(host, "gbl_cpu_", fn, args)
                assert row["host"][0] < 0 or early, (fn, name, row)
            table.append(row)
    with open(os.path.join(ROOT, "tests", "golden", "env_arg_errors.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in table) + "\n]\n")
    print(len(table), "cases")


if __name__ == "__main__":
    main()
