"""The contract of gbl_collect_search_tb (include/gobblet_hip.h, "Self-play with the tablebase"), ply by ply, on the oracle: the loop of
tests/noise_restatement.py's restate_collect_noise with the two additions -- the verdict of every judged ply and the TABLEBASE
mover -- built on a probe (`probe(state, to_move) -> {"outcome", "value", "action"}`: gbl_(cpu_)tb_probe, pinned by its own tests
against tests/tablebase_restatement.py) and on tests/tb_targets_restatement.py's sets R / S / O.  A plain module."""
import numpy as np

import oracle

from tests import noise_restatement as N
from tests import tb_targets_restatement as TR

NONE = -128
HOW_RANDOM, HOW_SEARCH, HOW_SEARCH_SAMPLED, HOW_PROVEN, HOW_TABLE, HOW_TABLE_SAMPLED = 0, 3, 4, 5, 6, 7


def table_row(outcome, value, mode, count):
    """The visits row of a TABLEBASE mover (count on O) and its value."""
    row = TR.targets(outcome[None], np.array([value]), np.array([0]), mode, count)["visits"][0]
    return row, TR.sign(int(value)) * 128 * int(row.sum())


def restate_collect_tb(probe, st, tm, turn, T, pols, nets, its, deps, noise, X, sample_plies, illegal_mode, seed, env_base, ply0, mode, count,
                       judge):
    """pols: "random" / "eval" / "tb" per side; judge: the three judge arrays are asked for.  Returns restate_collect_noise's tuple, the
    dict with "tb_outcomes" / "tb_value" / "tb_played" too (what the arrays hold when they are given)."""
    from tests.test_playout_policy import sample_stream
    from tests.test_selfplay_search import STREAM_VISIT, visits_draw
    from tests.test_selfplay_solve import NAMES, _solve_one
    n = len(st)
    st, tm, dn = st.copy(), tm.copy(), np.zeros(n, np.int8)
    turn = np.zeros(n, np.int32) if turn is None else turn.astype(np.int32).copy()
    out = {k: [] for k in [k for k, _, _ in NAMES] + ["tb_outcomes", "tb_value", "tb_played"]}
    for t in range(T):
        q = ply0 + t
        legal = oracle.batch_legal_mask(st, tm)
        actions, mover = np.zeros(n, np.int32), tm.copy()
        visits, value, nodes, how = np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int8)
        rootv, pri = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8)
        outcomes, proven = np.full((n, 54), NONE, np.int8), np.zeros(n, np.int8)
        tb_o, tb_v, tb_p = np.full((n, 54), NONE, np.int8), np.zeros(n, np.int8), np.full(n, NONE, np.int8)
        verdict = probe(st, tm) if judge or "tb" in pols else None  # (the position before the move, as its mover sees it; no mask)
        for b in range(n):
            m, g = int(tm[b]), env_base + b
            judged = judge or pols[m] == "tb"
            if judged:
                tb_o[b], tb_v[b] = verdict["outcome"][b], verdict["value"][b]
            if pols[m] == "tb" and int(verdict["action"][b]) >= 0:
                visits[b], value[b] = table_row(tb_o[b], int(tb_v[b]), mode, count)
                if turn[b] < sample_plies:
                    actions[b], how[b] = visits_draw(visits[b], N.word(seed, g, q, STREAM_VISIT)), HOW_TABLE_SAMPLED
                else:
                    actions[b], how[b] = int(verdict["action"][b]), HOW_TABLE
            elif pols[m] != "eval":  # RANDOM, or a TABLEBASE mover the table has no action for
                actions[b] = sample_stream(legal[b], seed, g, q, 0)
            else:
                mask = None
                done_ = False
                if deps[m] > 0 and legal[b].any():
                    outcomes[b], proven[b], a_star = _solve_one(st[b].tobytes(), m, deps[m])
                    if proven[b] != 0:  # no search, no draw
                        actions[b], how[b] = a_star, HOW_PROVEN
                        visits[b, a_star] = its[m]
                        value[b] = (1 if proven[b] > 0 else -1) * 128 * its[m]
                        done_ = True
                    mask = (outcomes[b] == 0).astype(np.int8)[None]
                if not done_:
                    v, w, l, a, nd, rv, rp, _ = N.restate_search_noise(nets[m], st[b:b + 1], tm[b:b + 1], mask, its[m], X, noise[m], seed, g, q)
                    visits[b], value[b], nodes[b], rootv[b], pri[b] = v[0], int((w[0] - l[0]).sum()), nd[0], rv[0], rp[0]
                    if turn[b] < sample_plies:
                        actions[b], how[b] = visits_draw(v[0], N.word(seed, g, q, STREAM_VISIT)), HOW_SEARCH_SAMPLED
                    else:
                        actions[b], how[b] = a[0], HOW_SEARCH
            if judged and actions[b] >= 0:
                tb_p[b] = tb_o[b, actions[b]]
        r = oracle.batch_step(st, tm, dn, actions, illegal_mode, auto_reset=True, turn=turn)
        for k, v in (("actions", actions), ("winner", r["winner"]), ("rewards", r["reward"]), ("done", dn.copy()), ("to_move", tm.copy()),
                     ("action_mask", r["mask"]), ("observation", r["obs"].reshape(n, 117)), ("visits", visits), ("value", value),
                     ("nodes", nodes), ("how", how), ("mover", mover), ("root_value", rootv), ("priors", pri), ("outcomes", outcomes),
                     ("proven", proven), ("tb_outcomes", tb_o), ("tb_value", tb_v), ("tb_played", tb_p)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, st, tm, dn, turn
