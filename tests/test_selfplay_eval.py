"""gbl_collect_search_eval on the host flavour (no GPU): whole games with the evaluator-guided search on either or both sides
against a Python loop over plies -- the restatement of gbl_tree_search_eval on the oracle (tests/evaluator_restatement.py), the
visit-proportional draw and generator word of tests/test_selfplay_search.py, and the oracle's step with auto-reset -- plus the
composition out of the host flavour's own entry points, properties, sharding, NULL outputs, tallies, the argument limits of both
flavours and the Python surface on device="cpu".

Two remarks on the cases.  (1) The entry point takes no root mask, and no board of the contract has an empty legal mask (a player's
two largest pieces can always go somewhere: only four cells can carry a largest piece on top; tests/positions.py's 3 754 boards
have at least 10 legal actions), so a candidate-less root cannot be put in front of it; the boards of tests/positions.py are in the
grid for what they are -- roots on which somebody already holds a line.  (2) Alignment rules belong to the device flavour, as
everywhere in the ABI: the host flavour reads host arrays a byte at a time."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests.positions import terminal_roots
from tests.search_harness import run
from tests.selfplay_harness import EVAL_NAMES as NAMES, _evaluator, host_collect, same
from tests.test_playout_policy import WIN_SEQ, UNCOVER_SEQ, play, random_midgames, sample_stream
from tests.test_selfplay_search import STREAM_VISIT, targets_numpy, visits_draw, word

SEARCH_ONLY = ("visits", "value", "nodes", "root_value", "priors")


def collect_eval(f, err, st, tm, turn, T, pols, nets, its, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev=None,
                 keep=None, counters=None):
    """gbl(_cpu)_collect_search_eval on host arrays; only the outputs named in `keep` are given (None: all).  Returns
    ({name: (T, n, ...)}, state, to_move, done, turn)."""
    return host_collect("eval", f, err, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev, keep,
                        counters, nets=nets, its=its)


def restate_collect(st, tm, turn, T, pols, nets, its, X, sample_plies, illegal_mode, seed, env_base, ply0):
    """The contract of gbl_collect_search_eval, ply by ply, on the oracle."""
    n = len(st)
    st, tm, dn = st.copy(), tm.copy(), np.zeros(n, np.int8)
    turn = np.zeros(n, np.int32) if turn is None else turn.astype(np.int32).copy()
    out = {k: [] for k, _, _ in NAMES}
    for t in range(T):
        q = ply0 + t
        legal = oracle.batch_legal_mask(st, tm)
        actions, mover = np.zeros(n, np.int32), tm.copy()
        visits, value, nodes, how = np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int8)
        rootv, pri = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8)
        for b in range(n):
            m, g = int(tm[b]), env_base + b
            if pols[m] == "eval":
                v, w, l, a, nd, rv, rp = R.restate_search(nets[m], st[b:b + 1], tm[b:b + 1], None, its[m], X)
                visits[b], value[b], nodes[b], rootv[b], pri[b] = v[0], int((w[0] - l[0]).sum()), nd[0], rv[0], rp[0]
                if turn[b] < sample_plies:
                    actions[b], how[b] = visits_draw(v[0], word(seed, g, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
                else:
                    actions[b], how[b] = a[0], nat.HOW_SEARCH
            else:
                actions[b] = sample_stream(legal[b], seed, g, q, 0)
        r = oracle.batch_step(st, tm, dn, actions, illegal_mode, auto_reset=True, turn=turn)
        for k, v in (("actions", actions), ("winner", r["winner"]), ("rewards", r["reward"]), ("done", dn.copy()), ("to_move", tm.copy()),
                     ("action_mask", r["mask"]), ("observation", r["obs"].reshape(n, 117)), ("visits", visits), ("value", value),
                     ("nodes", nodes), ("how", how), ("mover", mover), ("root_value", rootv), ("priors", pri)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, st, tm, dn, turn


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def nets():
    """player_1's network has 64 hidden units, player_2's 256."""
    return R.random_net(64, 69), R.random_net(256, 261)


@pytest.fixture(scope="module")
def boards(golden_dir):
    """Fresh boards, midgames of both movers, positions one ply from a decided game (a win to take, a line to uncover: games end and
    reset inside the window) and two of tests/positions.py's boards on which somebody holds a line already."""
    ms, mt = random_midgames(5, seed=5, min_plies=2, max_plies=14)
    (sw, mw), (su, mu) = play(WIN_SEQ), play(UNCOVER_SEQ)
    g = np.load(os.path.join(golden_dir, "board_functions.npz"))
    held = terminal_roots({"squares": g["squares"], "winner": g["winner"]}, n_random=200)[[0, -1]]
    st = np.concatenate([np.zeros((1, 27), np.int8), ms, sw[None], su[None], held, np.zeros((1, 27), np.int8)])
    tm = np.concatenate([[0], mt, [mw, mu], [0, 1], [0]]).astype(np.int8)
    turn = np.array([int((s != 0).sum()) for s in st], np.int32)  # (at least the pieces on the board)
    assert len(st) == 11 and set(tm.tolist()) == {0, 1} and (turn < 2).sum() >= 2 and (turn >= 2).sum() >= 5
    return np.ascontiguousarray(st), tm, turn


T = 5
GRID = list(itertools.product((("eval", "eval"), ("eval", "random"), ("random", "eval")), ((1, 3), (8, 8)), (0, 2),
                              (nat.ILLEGAL_NOOP, nat.ILLEGAL_TERMINATE)))


@pytest.fixture(scope="module")
def restated(boards, nets):
    """The restatement of every grid point, computed once (it does not depend on the layout or on how the ply index is split)."""
    st, tm, turn = boards
    memo = {}

    def get(pols, its, sample_plies, illegal_mode):
        key = (pols, its, sample_plies, illegal_mode)
        if key not in memo:
            memo[key] = restate_collect(st, tm, turn, T, pols, nets, its, 48, sample_plies, illegal_mode, 9, 7, 8)
        return memo[key]
    return get


@pytest.mark.parametrize("pols,its,sample_plies,illegal_mode", GRID)
def test_host_flavour_equals_restatement(cpu, boards, nets, restated, pols, its, sample_plies, illegal_mode):
    st, tm, turn = boards
    exp = restated(pols, its, sample_plies, illegal_mode)
    use = tuple(n if p == "eval" else None for n, p in zip(nets, pols))  # (NULL for a RANDOM side)
    for layout, ply_dev in (("time", None), ("tile", 3)):  # (ply0 + *ply_dev = 8 either way)
        got = collect_eval(cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error, st, tm, turn, T, pols, use, its, 48, sample_plies,
                           illegal_mode, layout, 9, 7, 8 - (ply_dev or 0), ply_dev)
        same(got, exp)
    assert exp[0]["done"].any()  # (games end inside the window: the boards one ply from a win)
    if sample_plies:
        assert (exp[0]["how"] == nat.HOW_SEARCH_SAMPLED).any() and (exp[0]["how"] == nat.HOW_SEARCH).any()


@pytest.fixture(scope="module")
def many():
    env = G.BatchedGobblet(200, "cpu", auto_reset=True, seed=11, track_turn=True)
    env.rollout(9)
    st, tm, turn = env.squares.numpy().copy(), env.to_move.numpy().copy(), env.turn.numpy().copy()
    assert (oracle.batch_winner(st) == 0).all()
    return st, tm, turn


def test_host_flavour_equals_composition(cpu, many, nets):
    """(eval, eval) without the opening draw is a loop of gbl_cpu_tree_search_eval + gbl_cpu_step_into."""
    st, tm, turn = many
    its, X, T_ = (24, 12), 32, 6
    got = collect_eval(cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error, st, tm, turn, T_, ("eval", "eval"), nets, its, X, 0,
                       nat.ILLEGAL_NOOP, "time", 1, 0, 0)
    n = len(st)
    s, m, d, tn = st.copy(), tm.copy(), np.zeros(n, np.int8), turn.copy()
    for t in range(T_):
        act, vis, val, nod, rv, pri = (np.zeros(n, np.int32), np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32),
                                       np.zeros(n, np.int32), np.zeros((n, 54), np.uint8))
        for side in (0, 1):
            idx = np.flatnonzero(m == side)
            if len(idx):
                v, w, l, a, nd, q, p = run("tree_search_eval", "cpu", s[idx], m[idx], None, (its[side], X), nets[side]).values()
                act[idx], vis[idx], val[idx], nod[idx], rv[idx], pri[idx] = a, v, (w - l).sum(1), nd, q, p
        win, rew = np.zeros(n, np.int8), np.zeros((n, 2), np.int8)
        mask, obs = np.zeros((n, 54), np.int8), np.zeros((n, 117), np.int8)
        rc = cpu.gbl_cpu_step_into(s.ctypes.data, m.ctypes.data, d.ctypes.data, act.ctypes.data, win.ctypes.data, rew.ctypes.data,
                                   mask.ctypes.data, obs.ctypes.data, tn.ctypes.data, None, None, None, n, nat.ILLEGAL_NOOP, 1, None)
        assert rc == 0, cpu.gbl_cpu_last_error()
        for k, v in (("actions", act), ("visits", vis), ("value", val), ("nodes", nod), ("root_value", rv), ("priors", pri), ("winner", win),
                     ("rewards", rew), ("done", d), ("to_move", m), ("action_mask", mask), ("observation", obs)):
            assert np.array_equal(got[0][k][t], v), (t, k)
    assert np.array_equal(got[1], s) and np.array_equal(got[4], tn)


def test_properties(cpu, many, nets):
    st, tm, turn = many
    its, sp = (24, 40), 3
    for pols in (("eval", "eval"), ("eval", "random"), ("random", "eval")):
        tr, s1, m1, d1, t1 = collect_eval(cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error, st, tm, turn, 10, pols, nets, its, 64, sp,
                                          nat.ILLEGAL_NOOP, "time", 3, 100, 0)
        mover, how, v, a = tr["mover"], tr["how"], tr["visits"].astype(np.int64), tr["actions"]
        srch = np.array([p == "eval" for p in pols])[mover]
        assert np.array_equal(how != nat.HOW_RANDOM, srch)
        # every root has candidates, so every iteration is a visit of a root child: the row sums to the iterations.  An iteration
        # either creates a node or reaches a terminal node again, so nodes - 1 is at most that sum, and equal to it while no terminal
        # node is reached twice (pinned below with one iteration per ply)
        assert (v.sum(2)[srch] == np.array(its)[mover][srch]).all() and (tr["nodes"][srch] - 1 <= v.sum(2)[srch]).all()
        assert (tr["nodes"][srch] >= 2).all()
        for k in SEARCH_ONLY:  # the RANDOM side's rows are zero
            assert (tr[k][~srch] == 0).all(), k
        # how is 4 exactly where turn < sample_plies on a searching side's ply (turn before ply t: replayed from the trajectory)
        before = np.zeros_like(mover, dtype=np.int64)
        cur = turn.astype(np.int64).copy()
        for t in range(10):
            before[t] = cur
            cur = np.where(tr["done"][t] != 0, 0, cur + 1)
        assert np.array_equal(cur, t1)
        assert np.array_equal(how == nat.HOW_SEARCH_SAMPLED, srch & (before < sp))
        picked = np.take_along_axis(v, a[..., None].astype(np.int64), 2)[..., 0]
        dec = how == nat.HOW_SEARCH
        assert (picked[dec] == v.max(2)[dec]).all() and (picked[how == nat.HOW_SEARCH_SAMPLED] > 0).all()
        # priors are zero outside the legal mask of the position searched: ply t's position is the one ply t - 1 left
        searched = np.concatenate([oracle.batch_legal_mask(st, tm)[None], tr["action_mask"][:-1]])
        assert (tr["priors"][searched == 0] == 0).all() and (tr["priors"][srch][searched[srch] != 0] >= 1).all()
        assert (np.abs(tr["value"]) <= v.sum(2) * 128).all() and (np.abs(tr["root_value"]) <= 128).all()
        assert np.array_equal(mover[0], tm) and np.array_equal(mover[1:], tr["to_move"][:-1])
        assert np.array_equal(m1, tr["to_move"][-1]) and np.array_equal(d1, tr["done"][-1])
    # the visits sum to nodes - 1 exactly while no visit reaches a terminal node again: one iteration per ply
    tr, *_ = collect_eval(cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error, st, tm, turn, 3, ("eval", "eval"), nets, (1, 1), 64, 0,
                          nat.ILLEGAL_NOOP, "time", 3, 100, 0)
    assert (tr["visits"].sum(2) == tr["nodes"] - 1).all() and (tr["nodes"] == 2).all()


def test_sharding(cpu, many, nets):
    st, tm, turn = many
    args = (6, ("eval", "random"), nets, (12, 12), 64, 2, nat.ILLEGAL_NOOP)
    f, err = cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error
    for layout in ("time", "tile"):
        whole = collect_eval(f, err, st, tm, turn, *args, layout, 3, 50, 2)
        a, k = 70, 90
        part = collect_eval(f, err, st[a:a + k], tm[a:a + k], turn[a:a + k], *args, layout, 3, 50 + a, 2)
        for key in whole[0]:
            assert np.array_equal(part[0][key], whole[0][key][:, a:a + k]), key
        for g, e in zip(part[1:], whole[1:]):
            assert np.array_equal(g, e[a:a + k])


def test_null_outputs_and_tallies(cpu, many, nets):
    st, tm, turn = many
    st, tm, turn = st[:70], tm[:70], turn[:70]
    f, err = cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error
    args = (4, ("eval", "eval"), nets, (6, 6), 64, 1, nat.ILLEGAL_NOOP, "time", 3, 0, 0)
    full = collect_eval(f, err, st, tm, turn, *args)
    optional = ("visits", "value", "nodes", "how", "mover", "root_value", "priors")
    for r in range(len(optional) + 1):  # every subset of the optional outputs, with and without the seven of gbl_collect
        for sub in itertools.combinations(optional, r):
            for base in ((), tuple(k for k, _, _ in NAMES[:7])):
                got = collect_eval(f, err, st, tm, turn, *args, keep=base + sub)
                assert set(got[0]) == set(base + sub)
                same(got, full)
    counters = np.zeros((nat.COUNTER_STRIPES, nat.COUNTER_STRIDE), np.int64)
    tr, *_ = collect_eval(f, err, st, tm, turn, 12, ("eval", "random"), nets, (8, 8), 64, 0, nat.ILLEGAL_NOOP, "time", 3, 0, 0,
                          keep=("done", "winner"), counters=counters)
    tot = counters.sum(0)
    assert tot[0] == 70 * 12 and tot[1] == tr["done"].sum() > 0
    assert tot[2] == (tr["winner"] == 1).sum() and tot[3] == (tr["winner"] == -1).sum()


# ---- argument limits ----------------------------------------------------------------------------------------------------------
def test_argument_limits():
    L, H = nat.cpu_raw(), nat.lib()  # (the device entry points check their arguments before any HIP call: no GPU needed)
    flavours = (("cpu", L.gbl_cpu_collect_search_eval, L.gbl_cpu_last_error), ("hip", H.gbl_collect_search_eval, H.gbl_last_error))
    n, T_ = 2, 2
    st, tm, dn = np.zeros((64, 27), np.int8), np.zeros(64, np.int8), np.zeros(64, np.int8)
    turn = np.zeros(64, np.int32)
    buf = np.zeros(64 * 1024, np.int8)
    base = (buf.ctypes.data + 15) & ~15
    net = R.random_net(64, 1)
    good = net.struct()
    assert all(p % 16 == 0 for p in (good.w1, good.b1, good.w2, good.b2))

    def ev(**kw):
        e = net.struct()
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    keepalive = []

    def call(f, p0=nat.POLICY_EVAL_TREE, p1=nat.POLICY_EVAL_TREE, e0=good, e1=good, I0=4, I1=4, X=64, sp=0, mode=0, ply0=0, plies=T_,
             env_base=0, n=n, ps=64, ts=64, turn=None, state=st.ctypes.data, actions=None, mask=None, visits=None, reward=None, rootv=None):
        keepalive.extend((e0, e1))
        return f(state, tm.ctypes.data, dn.ctypes.data, actions, None, reward, None, None, mask, None, visits, None, None, None, None, rootv,
                 None, n, ps, ts, 0, env_base, ply0, None, plies, p0, p1, None if e0 is None else C.addressof(e0),
                 None if e1 is None else C.addressof(e1), I0, I1, X, sp, mode, None, turn, None)

    bad_arg = [({"p0": nat.POLICY_TREE}, b"policy"), ({"p1": nat.POLICY_TREE}, b"policy"), ({"p0": nat.POLICY_GREEDY1}, b"policy"),
               ({"p1": nat.POLICY_GREEDY3}, b"policy"), ({"p0": 6}, b"policy"), ({"p1": -1}, b"policy"),
               ({"e0": None}, b"ev must not be NULL"), ({"e1": None}, b"ev must not be NULL"), ({"e0": ev(hidden=96)}, b"hidden"),
               ({"e1": ev(shift_p=25)}, b"shift"), ({"e0": ev(w1=None)}, b"w1 / b1 / w2 / b2 must not be NULL"),
               ({"I0": 0}, b"iterations"), ({"I1": 513}, b"iterations"), ({"X": 1025}, b"explore"), ({"X": -1}, b"explore"),
               ({"sp": -1}, b"sample_plies"), ({"sp": 2}, b"turn"), ({"mode": 2}, b"illegal_mode"),
               ({"ply0": (1 << 24) - 1}, b"2^24"), ({"ply0": 1 << 24, "plies": 1}, b"2^24"), ({"env_base": (1 << 42) - 1}, b"2^42"),
               ({"n": -1}, b"n < 0"), ({"state": None}, b"state"),
               ({"ps": 8}, b"stride"), ({"ps": 64, "ts": 64, "n": 65}, b"stride"), ({"ps": 72}, b"stride"), ({"ts": 0}, b"stride")]
    for kw, w in bad_arg:
        msgs = []
        for name, f, err in flavours:
            assert call(f, **kw) == nat.ERR_ARG, (name, kw)
            msgs.append(err())
            assert w in msgs[-1], (name, kw, msgs[-1])
        assert msgs[0] == msgs[1], kw  # the same message from both flavours
    for name, f, err in flavours:
        # a RANDOM side's evaluator and iterations are not read
        assert call(f, p1=nat.POLICY_RANDOM, e1=None, I1=0, n=0) == 0 and call(f, p0=nat.POLICY_RANDOM, e0=ev(hidden=96), I0=-5, n=0) == 0
        assert call(f, n=0) == 0 and call(f, plies=0) == 0, name
    # alignment is the device flavour's business (its row stores are 16-byte vectors, its weight loads dwords)
    _, f, err = flavours[1]
    for kw, w in (({"e0": ev(w1=good.w1 + 4)}, b"16-byte"), ({"e1": ev(b2=good.b2 + 8)}, b"16-byte"), ({"visits": base + 1}, b"visits_traj"),
                  ({"mask": base + 8}, b"mask_traj"), ({"actions": base + 2}, b"4-byte"), ({"rootv": base + 2}, b"4-byte"),
                  ({"reward": base + 1}, b"reward_traj"), ({"state": base + 4}, b"state")):
        assert call(f, **kw) == nat.ERR_ALIGN, kw
        assert w in err(), (kw, err())
    # the extremes are accepted (the host flavour runs them)
    _, f, err = flavours[0]
    assert call(f, turn=turn.ctypes.data, sp=2, I0=512, I1=1, X=1024, ply0=(1 << 24) - T_, env_base=(1 << 42) - n, actions=base) == 0, err()
    # gbl_collect_search and gbl_collect_policy refuse the new policy code, in both flavours
    hist = np.full((64, 2, 3), -1, np.int8)
    for cs, cp, err in ((L.gbl_cpu_collect_search, L.gbl_cpu_collect_policy, L.gbl_cpu_last_error),
                        (H.gbl_collect_search, H.gbl_collect_policy, H.gbl_last_error)):
        for p0, p1 in ((nat.POLICY_EVAL_TREE, 0), (0, nat.POLICY_EVAL_TREE), (nat.POLICY_EVAL_TREE, nat.POLICY_TREE)):
            assert cs(st.ctypes.data, tm.ctypes.data, dn.ctypes.data, *[None] * 12, n, 64, 64, 0, 0, 0, None, 1, p0, p1, 4, 4, 2, 2, 8, 64, 0, 0,
                      None, None, None) == nat.ERR_ARG
            assert b"policy" in err()
            assert cp(st.ctypes.data, tm.ctypes.data, dn.ctypes.data, hist.ctypes.data, *[None] * 10, n, 64, 64, 0, 0, 0, None, 1, p0, p1, 0, 0,
                      None, None, None) == nat.ERR_ARG
            assert b"policy" in err()
    assert nat.POLICY_EVAL_TREE == 5


# ---- the Python surface on device="cpu" -------------------------------------------------------------------------------------------
def test_python_surface_on_cpu(cpu, nets):
    ev0, ev1 = _evaluator(nets[0]), _evaluator(nets[1])
    env = G.BatchedGobblet(70, "cpu", auto_reset=True, seed=4, env_base=3, track_turn=True)
    env.rollout(5)
    st, tm, turn, ply = env.squares.numpy().copy(), env.to_move.numpy().copy(), env.turn.numpy().copy(), env.ply
    f, err = cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error

    def fresh():
        e = G.BatchedGobblet(70, "cpu", auto_reset=True, seed=4, env_base=3, track_turn=True)
        e.load_state_dict(env.state_dict())
        return e

    def check(out, exp, layout="time", plies=4):
        for k in exp[0]:
            v = out[k].numpy()
            if layout == "tile":  # (tiles, plies, 64, ...) -> (plies, n, ...)
                v = np.moveaxis(v, 1, 0).reshape((plies, -1) + v.shape[3:])[:, :70]
            assert np.array_equal(v.reshape(exp[0][k].shape), exp[0][k]), k
    # 1. the string, with search=: a pair of evaluators and of iterations
    for layout in ("time", "tile"):
        e = fresh()
        out = e.collect(4, policies=("evaluator", "evaluator"), layout=layout, count=True,
                        search=dict(evaluator=(ev0, ev1), iterations=(6, 3), explore=48, sample_plies=2))
        assert {"visits", "value", "nodes", "how", "mover", "root_value", "priors"} <= set(out) and e.ply == ply + 4
        assert out["root_value"].dtype == torch.int32 and out["priors"].dtype == torch.uint8 and out["priors"].shape[-1] == 54
        exp = collect_eval(f, err, st, tm, turn, 4, ("eval", "eval"), nets, (6, 3), 48, 2, nat.ILLEGAL_NOOP, layout, 4, 3, ply)
        check(out, exp, layout)
        assert np.array_equal(e.squares.numpy(), exp[1]) and np.array_equal(e.turn.numpy(), exp[4]) and int(e.counters[0]) == 70 * 4
        # 4. collect followed by outcome_targets
        e.outcome_targets(out)
        ez, el = targets_numpy(exp[0]["done"], exp[0]["rewards"], exp[0]["mover"])
        if layout == "time":
            assert np.array_equal(out["z"].numpy(), ez) and np.array_equal(out["plies_left"].numpy(), el)
    # 2. two policy instances supply evaluator, iterations and explore; buffers of the caller's own
    p0 = G.EvaluatorTreeSearchGobbletPolicy(ev0, iterations=5, explore=32)
    p1 = G.EvaluatorTreeSearchGobbletPolicy(ev1, iterations=2, explore=32)
    e = fresh()
    buf = e.trajectory_buffers(4, search_outputs=True, evaluator_outputs=True)
    out = e.collect(4, out=buf, policies=(p0, p1))
    check(out, collect_eval(f, err, st, tm, turn, 4, ("eval", "eval"), nets, (5, 2), 32, 0, nat.ILLEGAL_NOOP, "time", 4, 3, ply))
    # 3. "random" against an instance; one evaluator and one iterations value for "evaluator" against "random"
    out = fresh().collect(4, policies=("random", p1))
    check(out, collect_eval(f, err, st, tm, turn, 4, ("random", "eval"), (None, nets[1]), (0, 2), 32, 0, nat.ILLEGAL_NOOP, "time", 4, 3, ply))
    out = fresh().collect(4, policies=("evaluator", "random"), search=dict(evaluator=ev0, iterations=3))
    check(out, collect_eval(f, err, st, tm, turn, 4, ("eval", "random"), (nets[0], None), (3, 0), 16, 0, nat.ILLEGAL_NOOP, "time", 4, 3, ply))
    assert "evaluator" in G.BatchedGobblet.POLICIES and G._native.POLICY_EVAL_TREE == 5
    # the ValueErrors
    tree = G.TreeSearchGobbletPolicy(iterations=4, playouts=2, device="cpu")
    disagree = G.EvaluatorTreeSearchGobbletPolicy(ev1, iterations=2, explore=64)
    for bad, word_ in ((dict(policies=(p0, "tree")), "compose"), (dict(policies=(tree, p1)), "compose"), (dict(policies=("greedy", p0)), "compose"),
                       (dict(policies=("evaluator", "greedy3"), search=dict(evaluator=ev0)), "compose"),
                       (dict(policies=(p0, disagree)), "explore"), (dict(policies=("evaluator", "random")), "evaluator"),
                       (dict(policies=("evaluator", "evaluator"), search=dict(evaluator=ev0, iterations=600)), "iterations"),
                       (dict(policies=("evaluator", "evaluator"), search=dict(evaluator=ev0, playouts=4)), "unknown"),
                       (dict(policies=(p0, p1), opening_plies=2), "opening_plies")):
        with pytest.raises(ValueError, match=word_):
            e.collect(2, **bad)
    e.collect(2, policies=(p0, disagree), search=dict(explore=8))  # (an explicit value settles it)
    with pytest.raises(ValueError, match="track_turn"):
        G.BatchedGobblet(8, "cpu", auto_reset=True).collect(2, policies=(p0, p0), search=dict(sample_plies=1))
    # an evaluator on another device than the environment: a stand-in object on a device of its own
    elsewhere = _evaluator(nets[0])
    elsewhere.device = torch.device("cuda:0")
    with pytest.raises(ValueError, match="lives on"):
        e.collect(2, policies=("evaluator", "random"), search=dict(evaluator=elsewhere))
    # trajectory_buffers with and without evaluator_outputs
    plain, both = e.trajectory_buffers(3, search_outputs=True), e.trajectory_buffers(3, search_outputs=True, evaluator_outputs=True)
    assert "root_value" not in plain and "priors" not in plain and set(both) - set(plain) == {"root_value", "priors"}
    assert both["priors"].shape == (3, 70, 54) and both["root_value"].shape == (3, 70)
    with pytest.raises(ValueError):
        e.trajectory_buffers(3, evaluator_outputs=True)
    with pytest.raises(ValueError, match="unknown"):  # ("tree" keeps going to gbl_collect_search, which knows no evaluator)
        e.collect(2, policies=("tree", "tree"), search=dict(evaluator=ev0))


def test_example_runs_two_generations_on_the_host_flavour():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "examples/example_train_evaluator.py", "cpu", "--generations", "2", "--boards", "64", "--plies", "8",
                        "--steps", "20", "--games", "16", "--selfplay-iterations", "8", "--hidden", "64"], cwd=root, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "generation 2" in r.stdout and "arena" in r.stdout, r.stdout[-2000:]
