"""The playout cap of gbl_collect_search_cap restated from the header text alone (include/gobblet_hip.h), for tests/test_selfplay_cap.py:
the draw in plain Python integers on the oracle's Philox block (tests/noise_restatement.py's word), the ply's budget and weight, and
the window as a ply-by-ply loop composed of the host flavour's single-decision entry points -- gbl_cpu_solve,
gbl_cpu_tree_search_eval_noise (mask = C, the ply's budget and weight) and gbl_cpu_step_into -- which are pinned by their own
restatements and left as they are."""
import numpy as np

import oracle

from gobblet_rl_amd import _native as nat
from tests import noise_restatement as N
from tests import solver_restatement as SR
from tests.search_harness import run

STREAM_CAP, STREAM_VISIT = 9, 4
HOW_FAST, HOW_FAST_SAMPLED = 8, 9


def is_full(seed, g, q, share):
    """Whether ply q of board g is a full ply of a side with share `share` (in 1/256; 256: nothing is drawn)."""
    return share >= 256 or (N.word(seed, g, q, STREAM_CAP) >> 24) < share


def full_table(seed, boards, plies, share):
    """bool (len(plies), len(boards))."""
    return np.array([[is_full(seed, int(g), int(q), share) for g in boards] for q in plies])


def composed_loop(cpu, st, tm, turn, T, pols, nets, its, fast, share, deps, noise, X, sample_plies, seed, env_base, ply0):
    """The window, ply by ply.  Returns (plies: a list of {name: (n, ...)}, state, turn, roots: the (state, to_move) every ply started
    from)."""
    from tests.test_playout_policy import sample_stream
    from tests.test_selfplay_search import visits_draw
    n = len(st)
    s, m, d, tn = st.copy(), tm.copy(), np.zeros(n, np.int8), turn.astype(np.int32).copy()
    plies, roots = [], []
    for t in range(T):
        q = ply0 + t
        roots.append((s.copy(), m.copy()))
        legal = oracle.batch_legal_mask(s, m)
        act, vis, val, nod = np.zeros(n, np.int32), np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32)
        rv, pri, how = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8), np.zeros(n, np.int8)
        outcome, proven = np.full((n, 54), SR.NONE, np.int8), np.zeros(n, np.int8)
        for b in range(n):
            mv, g = int(m[b]), env_base + b
            if pols[mv] != "eval":
                act[b] = sample_stream(legal[b], seed, g, q, 0)
                continue
            mask = None
            if deps[mv] > 0:
                o, V, a_star = run("solve", "cpu", s[b:b + 1], m[b:b + 1], None, (deps[mv],)).values()
                outcome[b], proven[b] = o[0], V[0]
                if V[0] != 0:  # a proven ply stays as it is, whatever the draw says
                    act[b], how[b], vis[b, a_star[0]] = a_star[0], nat.HOW_PROVEN, its[mv]
                    val[b] = (1 if V[0] > 0 else -1) * 128 * its[mv]
                    continue
                mask = (o == 0).astype(np.int8)
            full = is_full(seed, g, q, share[mv])
            budget, weight = (its[mv], noise[mv]) if full else (fast[mv], 0)
            v, w, l, a, nd, rq, rp, _ = run("tree_search_eval_noise", "cpu", s[b:b + 1], m[b:b + 1], mask, (budget, X, weight, seed, g, q),
                                            nets[mv]).values()
            val[b], nod[b], rv[b], pri[b] = (w[0] - l[0]).sum(), nd[0], rq[0], rp[0]
            if full:
                vis[b] = v[0]  # (a fast ply's row stays 54 zeros)
            if tn[b] < sample_plies:
                act[b], how[b] = visits_draw(v[0], N.word(seed, g, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED if full else HOW_FAST_SAMPLED
            else:
                act[b], how[b] = a[0], nat.HOW_SEARCH if full else HOW_FAST
        mover = m.copy()
        win, rew = np.zeros(n, np.int8), np.zeros((n, 2), np.int8)
        mask_, obs = np.zeros((n, 54), np.int8), np.zeros((n, 117), np.int8)
        rc = cpu.gbl_cpu_step_into(s.ctypes.data, m.ctypes.data, d.ctypes.data, act.ctypes.data, win.ctypes.data, rew.ctypes.data,
                                   mask_.ctypes.data, obs.ctypes.data, tn.ctypes.data, None, None, None, n, nat.ILLEGAL_NOOP, 1, None)
        assert rc == 0, cpu.gbl_cpu_last_error()
        plies.append(dict(actions=act, visits=vis, value=val, nodes=nod, root_value=rv, priors=pri, how=how, outcomes=outcome, proven=proven,
                          mover=mover, winner=win, rewards=rew, done=d.copy(), to_move=m.copy(), action_mask=mask_, observation=obs))
    return plies, s, tn, roots
