"""``BatchedGobblet.collect``'s reading of ``policies=`` / ``search=`` for the self-play family (``gbl_collect_search`` and its
``_eval``, ``_solve``, ``_noise``, ``_cap``, ``_gumbel`` and ``_tb``, ``gbl_collect_gumbel_solve`` and ``gbl_collect_gumbel_tb``): which entry point a call takes, which trajectory buffers it
needs and the arguments the parse decides, by the names of ``_native.SELFPLAY_ARGS`` / ``SELFPLAY_ARGS_MORE`` / ``SELFPLAY_ARGS_TABLE``.  ``collect`` adds what belongs to the
environment (the boards, the buffers, the window, the counters, the stream) and calls.  What the keys mean: ``collect``'s docstring."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

from . import _native as nat

# a trajectory argument of the ABI -> the key of ``trajectory_buffers`` whose array it takes
TRAJ_BUFFERS = dict(actions_traj="actions", winner_traj="winner", reward_traj="rewards", done_traj="done", to_move_traj="to_move",
                    mask_traj="action_mask", obs_traj="observation", visits_traj="visits", value_traj="value", nodes_traj="nodes",
                    how_traj="how", mover_traj="mover", root_value_traj="root_value", priors_traj="priors", outcome_traj="outcomes",
                    proven_traj="proven", tb_outcome_traj="tb_outcomes", tb_value_traj="tb_value", tb_played_traj="tb_played")


class Plan(NamedTuple):
    entry: str | None  # the entry point, None: no side searches (gbl_collect_policy / gbl_collect_from_ex)
    outputs: dict      # trajectory_buffers' search_outputs / evaluator_outputs / solver_outputs / tablebase_outputs
    named: dict        # the arguments the parse decides, by the ABI's names
    alive: list        # the evaluator structs that named["ev0"] / ["ev1"] point to: kept until the call has returned


def plan(policies, search, device) -> Plan:
    """How ``collect(policies=, search=)`` of an environment on ``device`` is to be called."""
    tp = _tablebase_params(policies, search, device)  # None unless a side plays from the table or the table judges
    ep = tp["ep"] if tp is not None else _evaluator_params(policies, search, device)  # None unless a side plays the evaluator-guided search
    sp = ep if ep is not None else _search_params(policies, search)  # None unless a side plays a tree search
    guarded = ep is not None and any(ep["solve_depth"])  # (the solver in front of an evaluator side's searches)
    judged = tp is not None and tp["judge"]
    outputs = dict(search_outputs=sp is not None, evaluator_outputs=ep is not None, solver_outputs=guarded, tablebase_outputs=judged)
    if sp is None:
        return Plan(None, outputs, {}, [])
    named = dict(policy0=sp["policies"][0], policy1=sp["policies"][1], iterations0=sp["iterations"][0], iterations1=sp["iterations"][1],
                 explore=sp["explore"], sample_plies=sp["sample_plies"])
    if ep is None:
        return Plan("gbl_collect_search", outputs,
                    dict(named, playouts0=sp["playouts"][0], playouts1=sp["playouts"][1], max_plies=sp["max_plies"]), [])
    # the table inside the gumbel dict -> gbl_collect_gumbel_tb; a table side or the judge -> _tb; the Gumbel root rule -> _gumbel, with a solve depth of its own -> gbl_collect_gumbel_solve; a playout cap -> _cap; else any noise weight -> _noise (the
    # guarded kernel, whatever the depths), else any solve depth -> _solve, else _eval
    cap, gum = ep.get("cap"), ep.get("gumbel")
    if tp is not None:
        entry = "gbl_collect_gumbel_tb" if tp["inner"] else "gbl_collect_search_tb"
        if tp["inner"]:
            named.update(considered0=gum["considered"][0], considered1=gum["considered"][1], gumbel_noise=gum["noise"],
                         visit_offset=gum["visit_offset"], scale=gum["scale"])
        named.update(inventory=tp["inventory"], aux=tp["aux"], table=tp["table"], tb_mode=tp["mode"], tb_count=tp["count"])
        if not judged:  # (the three verdict arrays are the judge's: without it NULL, whatever the buffers hold)
            named.update(tb_outcome_traj=None, tb_value_traj=None, tb_played_traj=None)
    elif gum is not None:
        entry = "gbl_collect_gumbel_solve" if guarded else "gbl_collect_search_gumbel"
        named.update(considered0=gum["considered"][0], considered1=gum["considered"][1], gumbel_noise=gum["noise"],
                     visit_offset=gum["visit_offset"], scale=gum["scale"])
    elif cap is not None:
        entry = "gbl_collect_search_cap"
        named.update(fast_iterations0=cap["fast_iterations"][0], fast_iterations1=cap["fast_iterations"][1],
                     full_share0=cap["share"][0], full_share1=cap["share"][1])
    else:
        entry = "gbl_collect_search_noise" if any(ep["noise"]) else "gbl_collect_search_solve" if guarded else "gbl_collect_search_eval"
    structs = [None if e is None else e.as_struct() for e in ep["evaluators"]]
    ev0, ev1 = (None if st is None else C.addressof(st) for st in structs)
    sides = dict(ev0=ev0, ev1=ev1, solve_depth0=ep["solve_depth"][0], solve_depth1=ep["solve_depth"][1], noise0=ep["noise"][0], noise1=ep["noise"][1])
    # (an entry point without the depths or the weights was chosen because they are all 0)
    named.update({name: sides[name] for name, _ in nat.selfplay_table(entry) if name in sides})
    return Plan(entry, outputs, named, structs)


def _pair(v) -> list:
    """A per-side setting of ``search=``: a value for both sides, or a pair."""
    return list(v) if isinstance(v, (tuple, list)) else [v, v]


def _is_random(x) -> bool:
    return x == "random" or (not isinstance(x, str) and x == nat.POLICY_RANDOM)


def _search_kw(defaults: dict, search, unknown_msg: str) -> dict:
    """``defaults`` updated with ``search=``; a key it does not have is an error."""
    unknown = set(search or ()) - set(defaults)
    if unknown:
        raise ValueError(unknown_msg % sorted(unknown))
    return {**defaults, **(search or {})}


def _search_params(policies, search):
    """The arguments of ``gbl_collect_search`` when a side of ``policies`` plays the tree search, else None."""
    from .tree_policy import TreeSearchGobbletPolicy
    if policies is None or isinstance(policies, str):
        if search is not None:
            raise ValueError("search= belongs to policies with a 'tree' side")
        return None
    sides = list(policies)
    trees = [isinstance(x, TreeSearchGobbletPolicy) or x == "tree" or (not isinstance(x, str) and x == nat.POLICY_TREE) for x in sides]
    if len(sides) != 2 or not any(trees):
        if search is not None:
            raise ValueError("search= belongs to policies with a 'tree' side")
        return None
    kw = _search_kw(dict(iterations=256, playouts=16, max_plies=64, explore=16, sample_plies=0),  # TreeSearchGobbletPolicy's defaults
                    search, "search: unknown keys %s")
    its, pls = ([int(x) for x in _pair(kw[k])] for k in ("iterations", "playouts"))
    if len(its) != 2 or len(pls) != 2:
        raise ValueError("search: iterations / playouts are a value or a pair, one value per side")
    codes = []
    for m, x in enumerate(sides):
        if isinstance(x, TreeSearchGobbletPolicy):
            its[m], pls[m] = x.iterations, x.playouts
            if search is None or "max_plies" not in search:
                kw["max_plies"] = x.max_plies
            if search is None or "explore" not in search:
                kw["explore"] = x.explore
            codes.append(nat.POLICY_TREE)
        elif trees[m]:
            codes.append(nat.POLICY_TREE)
        elif _is_random(x):
            codes.append(nat.POLICY_RANDOM)
        else:
            raise ValueError("policies: the tree search plays against 'tree' or 'random' (not %r)" % (x,))
    for m in range(2):
        if codes[m] == nat.POLICY_TREE and not (1 <= its[m] <= 1024 and 1 <= pls[m] <= 256):
            raise ValueError("search: iterations must be in [1, 1024] and playouts in [1, 256]")
    if not (0 <= int(kw["max_plies"]) <= 255 and 0 <= int(kw["explore"]) <= 1024 and int(kw["sample_plies"]) >= 0):
        raise ValueError("search: max_plies must be in [0, 255], explore in [0, 1024], sample_plies >= 0")
    return dict(policies=codes, iterations=its, playouts=pls, max_plies=int(kw["max_plies"]), explore=int(kw["explore"]),
                sample_plies=int(kw["sample_plies"]))


def _evaluator_params(policies, search, device):
    """The arguments of ``gbl_collect_search_eval`` / ``_solve`` / ``_noise`` when a side of ``policies`` plays the evaluator-guided
    search, else None."""
    from .evaluator_policy import EvaluatorTreeSearchGobbletPolicy, GobbletEvaluator
    from .tree_policy import TreeSearchGobbletPolicy
    if policies is None or isinstance(policies, str):
        return None
    sides = list(policies)

    def is_eval(x):
        return isinstance(x, EvaluatorTreeSearchGobbletPolicy) or x == "evaluator" or \
            (not isinstance(x, (str, TreeSearchGobbletPolicy)) and x == nat.POLICY_EVAL_TREE)
    evs = [is_eval(x) for x in sides]
    if len(sides) != 2 or not any(evs):
        return None
    from .evaluator_policy import noise_weight
    kw = _search_kw(dict(evaluator=None, iterations=256, explore=None, sample_plies=0, solve_depth=0, noise=0.0, cap=None,
                         gumbel=None),  # EvaluatorTreeSearchGobbletPolicy's defaults
                    search, "search: unknown keys %s (an evaluator side takes evaluator / iterations / explore / sample_plies / "
                    "solve_depth / noise / cap / gumbel)")
    its, nets, deps, nzs = _pair(kw["iterations"]), _pair(kw["evaluator"]), _pair(kw["solve_depth"]), _pair(kw["noise"])
    if len(its) != 2 or len(nets) != 2 or len(deps) != 2 or len(nzs) != 2:
        raise ValueError("search: iterations / evaluator / solve_depth / noise are a value or a pair, one per side")
    nzs = [noise_weight(x or 0.0) for x in nzs]  # (shares in [0, 1] -> the ABI's weights 0 .. 256)
    codes, explores = [], []
    for m, x in enumerate(sides):
        if isinstance(x, EvaluatorTreeSearchGobbletPolicy):
            if x.gumbel is not None:
                raise ValueError("a policy instance with gumbel= does not bring its rule into collect(): pass 'evaluator' sides and "
                                 "search=dict(gumbel=...)")
            its[m], nets[m], nzs[m] = x.iterations, x.evaluator, x.noise
            explores.append(x.explore)
            codes.append(nat.POLICY_EVAL_TREE)
        elif evs[m]:
            codes.append(nat.POLICY_EVAL_TREE)
        elif _is_random(x):
            codes.append(nat.POLICY_RANDOM)
            nets[m] = None
        else:
            raise ValueError("policies: the evaluator-guided search plays against 'evaluator' or 'random' inside one launch (not %r); "
                             "against the tree search or a greedy policy, compose the loop: the policy's "
                             "compute_actions_from_state + step_into per ply" % (x,))
    if kw["explore"] is not None:
        explore = int(kw["explore"])
    elif explores:
        if len(set(explores)) > 1:
            raise ValueError("the two policy instances disagree on explore (%d, %d): one launch has one value; pass "
                             "search=dict(explore=...)" % tuple(explores))
        explore = explores[0]
    else:
        explore = 16
    for m in range(2):
        if codes[m] != nat.POLICY_EVAL_TREE:
            its[m] = deps[m] = nzs[m] = 0
            continue
        deps[m] = int(deps[m] or 0)
        if not 0 <= deps[m] <= nat.SOLVE_MAX_DEPTH:
            raise ValueError(f"search: solve_depth must be in [0, {nat.SOLVE_MAX_DEPTH}]")
        if not isinstance(nets[m], GobbletEvaluator):
            raise ValueError("search: an 'evaluator' side needs search=dict(evaluator=GobbletEvaluator ...)")
        if nat.device(nets[m].device) != nat.device(device):
            raise ValueError("the evaluator lives on %s and the environment on %s: move it with evaluator.to(...)"
                             % (nets[m].device, device))
        its[m] = int(its[m])
        if not 1 <= its[m] <= 512:
            raise ValueError("search: iterations must be in [1, 512]")
    if not (0 <= explore <= 1024 and int(kw["sample_plies"]) >= 0):
        raise ValueError("search: explore must be in [0, 1024], sample_plies >= 0")
    gumbel = _gumbel_params(kw["gumbel"], codes)
    if gumbel is not None and (any(deps) or any(nzs) or kw["cap"] is not None):
        raise ValueError("search: gumbel does not go with solve_depth, noise or cap beside it (the guard of a Gumbel side is "
                         "gumbel=dict(solve_depth=...): gbl_collect_gumbel_solve; the rule has no root noise and no cap)")
    if gumbel is not None:
        deps = gumbel.pop("solve_depth")
    return dict(policies=codes, evaluators=nets, iterations=its, explore=explore, sample_plies=int(kw["sample_plies"]),
                solve_depth=deps, noise=nzs, cap=_cap_params(kw["cap"], codes, its), gumbel=gumbel)


def _gumbel_params(gumbel, codes, keep=False):
    """``search=dict(gumbel=dict(considered=, noise=, visit_offset=, scale=, solve_depth=))`` as ``gbl_collect_search_gumbel`` and
    ``gbl_collect_gumbel_solve`` take it -- ``considered`` (0: that side keeps the search above) and ``solve_depth`` (the guard in front
    of that side's searches, 0: none) per side, the rest for both -- or None where no evaluator side follows the rule or is guarded
    through it (an absent ``gumbel``, ``considered=0`` without a depth): the call keeps its entry point.  ``keep``: the dict even then
    (``gbl_collect_gumbel_tb`` takes the rule's arguments whoever follows it)."""
    from .evaluator_policy import gumbel_args
    if gumbel is None:
        return None
    if not isinstance(gumbel, dict):
        raise ValueError("search: gumbel is a dict of considered / noise / visit_offset / scale / solve_depth")
    considered, depths = _pair(gumbel.get("considered", 16)), _pair(gumbel.get("solve_depth", 0))
    if len(considered) != 2 or len(depths) != 2:
        raise ValueError("search: gumbel's considered / solve_depth are a value or a pair, one per side")
    rest = gumbel_args({k: v for k, v in dict(gumbel, considered=1).items() if k != "solve_depth"})
    for m in range(2):
        if codes[m] != nat.POLICY_EVAL_TREE:
            considered[m] = depths[m] = 0
            continue
        if isinstance(considered[m], bool) or not 0 <= int(considered[m]) <= 54:
            raise ValueError("search: gumbel's considered must be in [0, 54]")
        if isinstance(depths[m], bool) or int(depths[m]) != depths[m] or not 0 <= int(depths[m]) <= nat.SOLVE_MAX_DEPTH:
            raise ValueError(f"search: gumbel's solve_depth must be in [0, {nat.SOLVE_MAX_DEPTH}]")
        considered[m], depths[m] = int(considered[m]), int(depths[m])
    if not any(considered) and not any(depths) and not keep:
        return None
    return dict(considered=considered, noise=rest["noise"], visit_offset=rest["visit_offset"], scale=rest["scale"], solve_depth=depths)


def _cap_params(cap, codes, its):
    """``search=dict(cap=dict(fast_iterations=, full=))`` as ``gbl_collect_search_cap`` takes it -- a fast budget and a share
    0 .. 256 per side -- or None where no evaluator side is capped (an absent ``cap``, ``full=1``): the call keeps its entry point."""
    from .evaluator_policy import cap_share
    if cap is None:
        return None
    if not isinstance(cap, dict) or set(cap) - {"fast_iterations", "full"}:
        raise ValueError("search: cap is a dict of fast_iterations / full")
    fast, full = _pair(cap.get("fast_iterations", 16)), _pair(cap.get("full", 0.25))
    if len(fast) != 2 or len(full) != 2:
        raise ValueError("search: cap's fast_iterations / full are a value or a pair, one per side")
    shares = [cap_share(x) for x in full]
    for m in range(2):
        if codes[m] != nat.POLICY_EVAL_TREE:
            fast[m], shares[m] = 0, nat.CAP_FULL_SHARE
        elif shares[m] < nat.CAP_FULL_SHARE:
            fast[m] = int(fast[m])
            if not 1 <= fast[m] <= its[m]:
                raise ValueError("search: cap's fast_iterations must be in [1, iterations]")
        else:
            fast[m] = 0
    if all(x == nat.CAP_FULL_SHARE for x in shares):
        return None
    return dict(fast_iterations=fast, share=shares)


def _tablebase_params(policies, search, device):
    """The table's arguments of ``gbl_collect_search_tb`` / ``gbl_collect_gumbel_tb`` and, under "ep", the rest of the call as
    ``_evaluator_params`` returns it (a table side stands there with its own policy code); None unless a side of ``policies`` plays
    from the table, ``search=dict(judge=True)``, or the table travels inside ``search=dict(gumbel=dict(tablebase=, judge=, ...))``
    ("inner": the Gumbel rule's entry point)."""
    from .evaluator_policy import GUMBEL_TABLE_KEYS
    from .tablebase import Tablebase, TablebaseGobbletPolicy
    if policies is None or isinstance(policies, str):
        return None
    sides = list(policies)

    def is_tb(x):
        return isinstance(x, TablebaseGobbletPolicy) or x == "tablebase" or \
            (isinstance(x, int) and not isinstance(x, bool) and x == nat.POLICY_TABLEBASE)
    tbs = [is_tb(x) for x in sides]
    search = search or {}
    gd = search.get("gumbel")
    inner = isinstance(gd, dict) and any(k in gd for k in GUMBEL_TABLE_KEYS)
    if inner:
        if len(sides) != 2:
            raise ValueError("search: gumbel's tablebase / judge belong to a pair of policies")
        if any(k in search for k in GUMBEL_TABLE_KEYS):
            raise ValueError("search: with the table inside gumbel=dict(...) (gbl_collect_gumbel_tb), tablebase / tb_mode / tb_count / "
                             "judge / allow_incomplete go inside that dict, not beside it")
        if any(_pair(gd.get("solve_depth", 0))):
            raise ValueError("search: gumbel's solve_depth does not go with tablebase / judge inside the dict (gbl_collect_gumbel_tb has "
                             "no solver guard)")
        if any(_pair(search.get("solve_depth", 0))) or any(_pair(search.get("noise", 0.0))):
            raise ValueError("search: gumbel does not go with solve_depth, noise or cap beside it (gbl_collect_gumbel_tb has none of them)")
    src = gd if inner else search
    judge = bool(src.get("judge", False))
    if len(sides) != 2 or not (any(tbs) or judge or inner):
        if search.get("tablebase") is not None:
            raise ValueError("search: tablebase= belongs to a pair of policies with a 'tablebase' side, or to judge=True")
        return None
    rest = {k: v for k, v in search.items() if k not in GUMBEL_TABLE_KEYS}
    if inner:  # (the rule's own keys stay for _gumbel_params)
        rest["gumbel"] = {k: v for k, v in gd.items() if k not in GUMBEL_TABLE_KEYS and k != "solve_depth"}
    kw = {**dict(tablebase=None, tb_mode="result", tb_count=1, allow_incomplete=False), **{k: v for k, v in src.items() if k in GUMBEL_TABLE_KEYS}}
    where = "search=dict(gumbel=dict(tablebase=Tablebase ...))" if inner else "search=dict(tablebase=Tablebase ...)"
    tb = kw["tablebase"]
    for x in sides:
        if isinstance(x, TablebaseGobbletPolicy):
            if tb is not None and tb is not x.tb:
                raise ValueError("one launch reads one table: the policy instance's and search=dict(tablebase=...) differ")
            tb = x.tb
    if not isinstance(tb, Tablebase):
        raise ValueError("search: a 'tablebase' side (or judge=True) needs " + where)
    if nat.device(tb.device) != nat.device(device):
        raise ValueError("the table lives on %s and the environment on %s" % (tb.device, device))
    if not tb.complete and not kw["allow_incomplete"]:
        raise ValueError("the table is not complete: a 0 would read 'not proven yet' (allow_incomplete=True to play from it anyway)")
    if kw["tb_mode"] not in nat.TB_TARGET_MODES:
        raise ValueError("search: tb_mode is 'result' or 'shortest'")
    if not 1 <= int(kw["tb_count"]) <= nat.TB_TARGET_MAX_COUNT:
        raise ValueError("search: tb_count must be in [1, %d]" % nat.TB_TARGET_MAX_COUNT)
    if rest.get("cap") is not None:
        raise ValueError("search: cap does not go with a 'tablebase' side or judge=True (neither gbl_collect_search_tb nor "
                         "gbl_collect_gumbel_tb has a playout cap)")
    if rest.get("gumbel") is not None and not inner:
        raise ValueError("search: gumbel does not go with a 'tablebase' side or judge=True beside it (gbl_collect_search_tb has no Gumbel "
                         "rule; the table of a Gumbel window travels inside the dict: gumbel=dict(tablebase=..., judge=...))")
    others = ["random" if t else x for t, x in zip(tbs, sides)]
    ep = _evaluator_params(others, rest or None, device)
    if ep is None:  # no evaluator side: the table against itself or against "random"
        if not all(_is_random(x) for x in others):
            raise ValueError("policies: the table plays against 'tablebase', 'evaluator' or 'random' inside one launch (not %r)" % (sides,))
        unknown = set(rest) - {"sample_plies", "evaluator", "iterations", "explore", "solve_depth", "noise", "cap", "gumbel"}
        if unknown:
            raise ValueError("search: unknown keys %s" % sorted(unknown))
        if int(rest.get("sample_plies", 0)) < 0:
            raise ValueError("search: sample_plies >= 0")
        ep = dict(policies=[nat.POLICY_RANDOM] * 2, evaluators=[None, None], iterations=[0, 0], explore=16,
                  sample_plies=int(rest.get("sample_plies", 0)), solve_depth=[0, 0], noise=[0, 0], cap=None, gumbel=None)
    if inner and ep["gumbel"] is None:  # (no side follows the rule: its arguments travel all the same, checked)
        ep["gumbel"] = _gumbel_params(rest["gumbel"], ep["policies"], keep=True)
        ep["gumbel"].pop("solve_depth")
    ep["policies"] = [nat.POLICY_TABLEBASE if t else c for t, c in zip(tbs, ep["policies"])]
    return dict(ep=ep, judge=judge, inner=inner, tb=tb, inventory=tb._inv, aux=tb._aux.data_ptr(), table=tb.table.data_ptr(),
                mode=nat.TB_TARGET_MODES[kw["tb_mode"]], count=int(kw["tb_count"]))
