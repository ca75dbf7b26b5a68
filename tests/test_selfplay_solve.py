"""gbl_collect_search_solve on the host flavour (no GPU): evaluator self-play with the exact solver in front of every search.
Against a ply-by-ply Python restatement of the contract (tests/solver_restatement.py decides what is proven,
tests/evaluator_restatement.py searches the unproven actions, the oracle steps); against the composed host loop gbl_cpu_solve +
gbl_cpu_tree_search_eval(mask = C) + gbl_cpu_step_into, with all three branches counted; depths (0, 0) against
gbl_cpu_collect_search_eval; the guard's property, read off the trajectory alone; the argument errors of both flavours; and the
one-hot rows a trainer gets from training_batch.

Positions: the fixture of every search test, BatchedGobblet(..., seed=11, track_turn=True).rollout(64) (board b depends on b alone, so
the first boards of a small environment are the first boards of the large one).  Network: smoke()'s seeded integer evaluator."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests import solver_restatement as SR
from tests.search_harness import midgame_boards, run
from tests.selfplay_harness import SOLVE_NAMES as NAMES, host_collect, same
from tests.test_playout_policy import sample_stream
from tests.test_selfplay_eval import collect_eval
from tests.test_selfplay_search import STREAM_VISIT, visits_draw, word

EXPLORE = 48


def smoke_net():
    """smoke()'s network: default_rng(0), 64 hidden units, shifts 1, 9, 9."""
    rng = np.random.default_rng(0)
    return R.Net(rng.integers(-128, 128, (117, 64), dtype=np.int8), rng.integers(-300, 300, 64).astype(np.int32),
                 rng.integers(-128, 128, (16, 56, 4), dtype=np.int8), rng.integers(-65536, 65536, 56).astype(np.int32), 1, 9, 9)


def fixture_boards(n, device="cpu"):
    return midgame_boards(n, device, turn=True)


def six_boards(c5):
    """2 empty boards + 4 of the fixture, some of them inside the sampled plies."""
    st = np.concatenate([np.zeros((2, 27), np.int8), c5[0][:4]])
    tm = np.concatenate([np.zeros(2, np.int8), c5[1][:4]])
    turn = np.concatenate([np.zeros(2, np.int32), c5[2][:4] % 4])
    return st, tm, turn


def collect_solve(f, err, st, tm, turn, T, pols, nets, its, deps, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev=None,
                  keep=None, noise=None):
    """gbl_cpu_collect_search_solve (with `noise`, a pair of weights: gbl_cpu_collect_search_noise) on host arrays, as
    tests/test_selfplay_eval.py's collect_eval: ({name: (T, n, ...)}, state, to_move, done, turn)."""
    return host_collect("solve" if noise is None else "noise", f, err, st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed,
                        env_base, ply0, ply_dev, keep, nets=nets, its=its, deps=deps, noise=noise or (0, 0))


@functools.lru_cache(maxsize=None)
def _solve_one(state_bytes, mover, depth):
    o, v, a = SR.solve(np.frombuffer(state_bytes, np.int8)[None], np.array([mover], np.int8), None, depth)
    return o[0], int(v[0]), int(a[0])


def restate_collect_solve(st, tm, turn, T, pols, nets, its, deps, X, sample_plies, illegal_mode, seed, env_base, ply0):
    """The contract of gbl_collect_search_solve, ply by ply, on the oracle: restate_collect of tests/test_selfplay_eval.py with the
    solver's three cases in front of the search."""
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
        outcomes, proven = np.full((n, 54), SR.NONE, np.int8), np.zeros(n, np.int8)
        for b in range(n):
            m, g = int(tm[b]), env_base + b
            if pols[m] != "eval":
                actions[b] = sample_stream(legal[b], seed, g, q, 0)
                continue
            mask = None
            if deps[m] > 0 and legal[b].any():
                outcomes[b], proven[b], a_star = _solve_one(st[b].tobytes(), m, deps[m])
                if proven[b] != 0:  # a forced win, or nothing but forced losses: no search, no draw
                    actions[b], how[b] = a_star, nat.HOW_PROVEN
                    visits[b, a_star] = its[m]
                    value[b] = (1 if proven[b] > 0 else -1) * 128 * its[m]
                    continue
                mask = (outcomes[b] == 0).astype(np.int8)[None]
                assert mask.any()
            v, w, l, a, nd, rv, rp = R.restate_search(nets[m], st[b:b + 1], tm[b:b + 1], mask, its[m], X)
            visits[b], value[b], nodes[b], rootv[b], pri[b] = v[0], int((w[0] - l[0]).sum()), nd[0], rv[0], rp[0]
            if turn[b] < sample_plies:
                actions[b], how[b] = visits_draw(v[0], word(seed, g, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
            else:
                actions[b], how[b] = a[0], nat.HOW_SEARCH
        r = oracle.batch_step(st, tm, dn, actions, illegal_mode, auto_reset=True, turn=turn)
        for k, v in (("actions", actions), ("winner", r["winner"]), ("rewards", r["reward"]), ("done", dn.copy()), ("to_move", tm.copy()),
                     ("action_mask", r["mask"]), ("observation", r["obs"].reshape(n, 117)), ("visits", visits), ("value", value),
                     ("nodes", nodes), ("how", how), ("mover", mover), ("root_value", rootv), ("priors", pri), ("outcomes", outcomes),
                     ("proven", proven)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, st, tm, dn, turn


# the restatement's cases: (policies, depths, iterations); the issue's depths (2, 3) and (3, 0), and a RANDOM side
CASES = ((("eval", "eval"), (2, 3), (8, 3)), (("eval", "eval"), (3, 0), (8, 3)), (("eval", "random"), (3, 2), (3, 0)),
         (("random", "eval"), (0, 2), (0, 8)))
T = 5
WINDOW = dict(seed=9, env_base=(1 << 40) - 20, ply0=8)


@functools.lru_cache(maxsize=None)
def restated_six(case, sample_plies, illegal_mode):
    """The restatement of a case on the six boards, computed once for the CPU and the GPU tests."""
    pols, deps, its = CASES[case]
    st, tm, turn = six_boards(fixture_boards(4))
    net = smoke_net()
    return restate_collect_solve(st, tm, turn, T, pols, (net, net), its, deps, EXPLORE, sample_plies, illegal_mode, WINDOW["seed"],
                                 WINDOW["env_base"], WINDOW["ply0"])


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def c5():
    return fixture_boards(65)


@pytest.mark.parametrize("illegal_mode", [nat.ILLEGAL_NOOP, nat.ILLEGAL_TERMINATE])
@pytest.mark.parametrize("sample_plies", [0, 2])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_flavour_equals_restatement(cpu, c5, case, sample_plies, illegal_mode):
    pols, deps, its = CASES[case]
    st, tm, turn = six_boards(c5)
    net = smoke_net()
    exp = restated_six(case, sample_plies, illegal_mode)
    use = tuple(net if p == "eval" else None for p in pols)  # (NULL for a RANDOM side)
    for layout, ply_dev in (("time", None), ("tile", 3)):
        got = collect_solve(cpu.gbl_cpu_collect_search_solve, cpu.gbl_cpu_last_error, st, tm, turn, T, pols, use, its, deps, EXPLORE,
                            sample_plies, illegal_mode, layout, WINDOW["seed"], WINDOW["env_base"], WINDOW["ply0"] - (ply_dev or 0), ply_dev)
        same(got, exp)
    how, mover = exp[0]["how"], exp[0]["mover"]
    guarded = np.array([p == "eval" and d > 0 for p, d in zip(pols, deps)])[mover]
    assert (exp[0]["outcomes"][~guarded] == SR.NONE).all() and (exp[0]["proven"][~guarded] == 0).all()
    assert ((how == nat.HOW_PROVEN) == (exp[0]["proven"] != 0)).all() and (exp[0]["outcomes"][guarded] != SR.NONE).any()
    if sample_plies and "random" not in pols:
        assert (how == nat.HOW_SEARCH_SAMPLED).any()


def composed_loop(cpu, net, st, tm, turn, T_, its, depth, X):
    """gbl_cpu_solve + gbl_cpu_tree_search_eval(mask = C) + gbl_cpu_step_into per ply, both sides guarded at `depth`: the arrays per
    ply, the final state and turn, and the plies of each branch (proven wins, proven losses, searched)."""
    n = len(st)
    s, m, d, tn = st.copy(), tm.copy(), np.zeros(n, np.int8), turn.copy()
    plies, tally = [], np.zeros(3, np.int64)
    for _ in range(T_):
        outcome, V, a_star = run("solve", "cpu", s, m, None, (depth,)).values()
        act, vis, val, nod = a_star.copy(), np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32)
        rv, pri, how = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8), np.full(n, nat.HOW_PROVEN, np.int8)
        won, lost = V > 0, V < 0
        vis[np.flatnonzero(V != 0), a_star[V != 0]] = its
        val[won], val[lost] = 128 * its, -128 * its
        idx = np.flatnonzero(V == 0)
        if len(idx):
            C_ = (outcome[idx] == 0).astype(np.int8)
            assert C_.any(1).all()
            v, w, l, a, nd, q, p = run("tree_search_eval", "cpu", s[idx], m[idx], C_, (its, X), net).values()
            act[idx], vis[idx], val[idx], nod[idx], rv[idx], pri[idx], how[idx] = a, v, (w - l).sum(1), nd, q, p, nat.HOW_SEARCH
        tally += (won.sum(), lost.sum(), len(idx))
        win, rew = np.zeros(n, np.int8), np.zeros((n, 2), np.int8)
        mask, obs = np.zeros((n, 54), np.int8), np.zeros((n, 117), np.int8)
        rc = cpu.gbl_cpu_step_into(s.ctypes.data, m.ctypes.data, d.ctypes.data, act.ctypes.data, win.ctypes.data, rew.ctypes.data,
                                   mask.ctypes.data, obs.ctypes.data, tn.ctypes.data, None, None, None, n, nat.ILLEGAL_NOOP, 1, None)
        assert rc == 0, cpu.gbl_cpu_last_error()
        plies.append(dict(actions=act, visits=vis, value=val, nodes=nod, root_value=rv, priors=pri, how=how, outcomes=outcome, proven=V,
                          winner=win, rewards=rew, done=d.copy(), to_move=m.copy(), action_mask=mask, observation=obs))
    return plies, s, tn, tally


@pytest.mark.parametrize("depth", [2, 3])
def test_host_flavour_equals_composed_loop(cpu, c5, depth):
    st, tm, turn = c5
    net, its, T_ = smoke_net(), 8, 6
    got = collect_solve(cpu.gbl_cpu_collect_search_solve, cpu.gbl_cpu_last_error, st, tm, turn, T_, ("eval", "eval"), (net, net), (its, its),
                        (depth, depth), EXPLORE, 0, nat.ILLEGAL_NOOP, "time", 1, 0, 0)
    plies, s, tn, tally = composed_loop(cpu, net, st, tm, turn, T_, its, depth, EXPLORE)
    for t, ply in enumerate(plies):
        for k, v in ply.items():
            assert np.array_equal(got[0][k][t], v), (t, k)
    assert np.array_equal(got[1], s) and np.array_equal(got[4], tn)
    print("depth %d: proven wins / proven losses / searched = %d / %d / %d" % (depth, *tally))
    assert tally.sum() == 65 * T_ and (tally >= 5).all(), tally  # all three branches were exercised


def test_depths_zero_is_collect_search_eval(cpu, c5):
    st, tm, turn = c5[0][:20], c5[1][:20], c5[2][:20] % 4
    net = smoke_net()
    for pols, its in ((("eval", "eval"), (8, 3)), (("random", "eval"), (0, 5))):
        use = tuple(net if p == "eval" else None for p in pols)
        for layout in ("time", "tile"):
            got = collect_solve(cpu.gbl_cpu_collect_search_solve, cpu.gbl_cpu_last_error, st, tm, turn, 4, pols, use, its, (0, 0), EXPLORE, 2,
                                nat.ILLEGAL_TERMINATE, layout, 3, 17, 4)
            exp = collect_eval(cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error, st, tm, turn, 4, pols, use, its, EXPLORE, 2,
                               nat.ILLEGAL_TERMINATE, layout, 3, 17, 4)
            assert (got[0].pop("outcomes") == SR.NONE).all() and (got[0].pop("proven") == 0).all()
            same(got, exp)


def guard_property(cpu, tr, st, tm, deps):
    """For every ply a guarded side moved: the position from the mover's observation (the slot before; the start for ply 0), solved
    again by gbl_cpu_solve -- a proven win is taken by its shortest line, and no proven loss is played beside an unproven action."""
    T_, n = tr["actions"].shape
    wins = avoided = 0
    for t in range(T_):
        if t == 0:
            s, m = st, tm
        else:
            obs = np.ascontiguousarray(tr["observation"][t - 1])
            s, m = np.zeros((n, 27), np.int8), np.zeros(n, np.int8)
            assert cpu.gbl_cpu_decode_obs(obs.ctypes.data, s.ctypes.data, m.ctypes.data, n, None) == 0
        assert np.array_equal(m != 0, tr["mover"][t] != 0)
        for side in (0, 1):
            idx = np.flatnonzero((m != 0) == bool(side))
            if not deps[side] or not len(idx):
                continue
            outcome = run("solve", "cpu", s[idx], m[idx], None, (deps[side],))["outcome"].astype(np.int64)
            a = tr["actions"][t][idx]
            played = outcome[np.arange(len(idx)), a]
            assert (played != SR.NONE).all()
            pos = np.where(outcome > 0, outcome, 1000)
            has_win = (outcome > 0).any(1)
            assert (played[has_win] == pos.min(1)[has_win]).all(), t
            open_ = (outcome == 0).any(1)
            assert (played[open_] >= 0).all(), t
            wins += has_win.sum()
            avoided += (open_ & (outcome < 0).any(1) & ~has_win).sum()
    return wins, avoided


def test_guard_property(cpu, c5):
    st, tm, turn = c5
    net = smoke_net()
    for deps, pols, sp in (((3, 2), ("eval", "eval"), 3), ((2, 0), ("eval", "random"), 0)):
        use = tuple(net if p == "eval" else None for p in pols)
        tr, *_ = collect_solve(cpu.gbl_cpu_collect_search_solve, cpu.gbl_cpu_last_error, st, tm, turn % 6, 8, pols, use, (8, 8), deps, EXPLORE,
                               sp, nat.ILLEGAL_NOOP, "time", 5, 0, 0)
        wins, avoided = guard_property(cpu, tr, st, tm, deps)
        assert wins >= 5 and avoided >= 5, (wins, avoided)  # (the property was put to the test)


def test_argument_errors():
    L, H = nat.cpu_raw(), nat.lib()  # (the device entry point checks its arguments before any HIP call: no GPU needed)
    st, tm, dn = np.zeros((64, 27), np.int8), np.zeros(64, np.int8), np.zeros(64, np.int8)
    good = smoke_net().struct()

    def call(f, p0=nat.POLICY_EVAL_TREE, p1=nat.POLICY_EVAL_TREE, e0=good, e1=good, d0=2, d1=2, n=2):
        return f(st.ctypes.data, tm.ctypes.data, dn.ctypes.data, *[None] * 16, n, 64, 64, 0, 0, 0, None, 2, p0, p1,
                 None if e0 is None else C.addressof(e0), None if e1 is None else C.addressof(e1), 4, 4, d0, d1, 64, 0, 0, None, None, None)
    for name, f, err in (("cpu", L.gbl_cpu_collect_search_solve, L.gbl_cpu_last_error), ("hip", H.gbl_collect_search_solve, H.gbl_last_error)):
        for kw, w in (({"d0": 7}, b"solve_depth"), ({"d1": 7}, b"solve_depth"), ({"d0": -1}, b"solve_depth"), ({"d1": -1}, b"solve_depth"),
                      ({"e0": None}, b"ev must not be NULL"), ({"e1": None, "d0": 0}, b"ev must not be NULL"),
                      ({"p0": nat.POLICY_TREE}, b"policy")):
            assert call(f, **kw) == nat.ERR_ARG, (name, kw)
            assert w in err(), (name, kw, err())
        # a RANDOM side's depth, evaluator and iterations are not read; the extremes pass
        assert call(f, p1=nat.POLICY_RANDOM, e1=None, d1=99, n=0) == 0 and call(f, d0=0, d1=nat.SOLVE_MAX_DEPTH, n=0) == 0, name
    assert nat.HOW_PROVEN == 5


def test_python_surface_and_one_hot_rows(c5):
    net = smoke_net()
    ev = G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, 1, 9, 9, device="cpu")
    L = nat.cpu_raw()

    def fresh():
        e = G.BatchedGobblet(65, "cpu", auto_reset=True, seed=11, track_turn=True)
        e.rollout(64)
        return e
    env = fresh()
    st, tm, turn, ply = env.squares.numpy().copy(), env.to_move.numpy().copy(), env.turn.numpy().copy(), env.ply
    its = 8
    traj = env.collect(6, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=its, solve_depth=(3, 2), explore=EXPLORE))
    assert traj["outcomes"].shape == (6, 65, 54) and traj["outcomes"].dtype == torch.int8
    assert traj["proven"].shape == (6, 65) and traj["proven"].dtype == torch.int8
    exp = collect_solve(L.gbl_cpu_collect_search_solve, L.gbl_cpu_last_error, st, tm, turn, 6, ("eval", "eval"), (net, net), (its, its), (3, 2),
                        EXPLORE, 0, nat.ILLEGAL_NOOP, "time", 11, 0, ply)
    for k in exp[0]:
        assert np.array_equal(traj[k].numpy().reshape(exp[0][k].shape), exp[0][k]), k
    # one depth for both sides, the tile layout; depth 0 / absent take the unguarded path and add nothing
    e2 = fresh()
    t2 = e2.collect(6, policies=("evaluator", "evaluator"), layout="tile", search=dict(evaluator=ev, iterations=its, solve_depth=2, explore=EXPLORE))
    assert t2["outcomes"].shape == (2, 6, 64, 54) and (t2["how"] == nat.HOW_PROVEN).any()
    for sd in ({}, {"solve_depth": 0}, {"solve_depth": (0, 0)}):
        t3 = fresh().collect(2, policies=("evaluator", "random"), search=dict(evaluator=ev, iterations=2, **sd))
        assert "outcomes" not in t3 and "proven" not in t3
    with pytest.raises(ValueError, match="solve_depth"):
        fresh().collect(2, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=2, solve_depth=7))
    with pytest.raises(ValueError):
        env.trajectory_buffers(3, search_outputs=True, solver_outputs=True)
    # outcome_targets and training_batch take the window as it is: a PROVEN ply's row sums to the iterations, on one action
    env.outcome_targets(traj)
    batch = env.training_batch(traj, 512, symmetries="all", call=1)
    idx = batch["index"].numpy()
    ok = idx[:, 0] >= 0
    how = traj["how"].numpy()[idx[ok, 0], idx[ok, 1]]
    rows = batch["visits"].numpy()[ok].astype(np.int64)
    proven = how == nat.HOW_PROVEN
    assert proven.sum() >= 5 and (rows[proven].sum(1) == its).all() and ((rows[proven] != 0).sum(1) == 1).all()
    assert (rows.sum(1) == its).all()
