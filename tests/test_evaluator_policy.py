"""gbl_evaluate / gbl_tree_search_eval / GobbletEvaluator / EvaluatorTreeSearchGobbletPolicy on the host flavour (no GPU): against
the Python restatement of the header text (tests/evaluator_restatement.py), plus properties, tactics with the zero evaluator, the
recorded argument errors and the quantiser."""
import json
import math
import os

import numpy as np
import pytest
import torch

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests.positions import terminal_roots
from tests.search_harness import replay_arg_errors, run, same
from tests.test_playout_policy import UNCOVER_ACTION, UNCOVER_SEQ, WIN_ACTION, WIN_SEQ, play, random_midgames
from tests.test_tree_policy import threat_positions, winning_moves

DEFAULT_EXPLORE = 16  # (the best of the sweep in profiles/r10/evaluator_policy.json)


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def positions(golden_dir):
    """tests/positions.py's boards on which somebody holds a line (a slice of them, both movers), fresh boards and midgames."""
    term = terminal_roots(np.load(os.path.join(golden_dir, "board_functions.npz")), n_random=400)[:24]
    ms, mt = random_midgames(24, seed=21, max_plies=20)
    st = np.concatenate([np.zeros((2, 27), np.int8), term, ms])
    tm = np.concatenate([np.array([0, 1], np.int8), (np.arange(len(term)) & 1).astype(np.int8), mt])
    assert len(st) == 50 and set(tm.tolist()) == {0, 1}
    return np.ascontiguousarray(st), np.ascontiguousarray(tm)


def nets(hidden):
    return {"random": R.random_net(hidden, 5 + hidden), "max": R.extreme_net(hidden, 1, 1), "min": R.extreme_net(hidden, -1, -1),
            "mixed": R.extreme_net(hidden, 1, -1), "zero": R.zero_net(hidden)}


@pytest.mark.parametrize("hidden", [64, 256])
def test_evaluate_equals_restatement(cpu, positions, hidden):
    st, tm = positions
    mask = (np.random.default_rng(3).random((len(st), 54)) < 0.4).astype(np.int8)
    mask[4] = 0  # a board without a candidate
    for kind, net in nets(hidden).items():
        exp = R.restate_evaluate(net, st, tm)
        same(run("evaluate", "cpu", st, tm, None, (), net), exp)
        got = run("evaluate", "cpu", st, tm, mask, (), net)
        same(got, R.restate_evaluate(net, st, tm, mask))
        assert not got["priors"][4].any() and got["value"][4] == exp[1][4]  # no candidate: zero priors, the value all the same
        assert np.array_equal(run("evaluate", "cpu", st, tm, None, (), net, keep=("priors", "value"))["priors"], exp[0]), kind
        legal = oracle.batch_legal_mask(st, tm) != 0
        assert ((exp[0] > 0) == legal).all()
        if kind == "zero":  # uniform priors, value 0
            cnt = legal.sum(1)
            assert (exp[1] == 0).all() and (exp[2] == 0).all()
            assert all((exp[0][b][legal[b]] == 1 + 254 // cnt[b]).all() for b in range(len(st)) if cnt[b])
        if kind == "random":  # the shift leaves hidden units clamped at 0, clamped at 127 and in between
            pre = np.concatenate([R.hidden_sums(net, s, int(m != 0)) >> net.shift1 for s, m in zip(st, tm)])
            low, high = int((pre <= 0).sum()), int((pre >= 127).sum())
            print("hidden units clamped at 0: %d, at 127: %d, in between: %d" % (low, high, len(pre) - low - high))
            assert low > len(pre) // 20 and high > len(pre) // 20 and len(pre) - low - high > len(pre) // 20
        if kind in ("max", "mixed"):  # every hidden unit at 127, every output at its largest magnitude: still inside int32
            assert abs(int(exp[2][0, 0])) == (1 << 24) + hidden * 127 * (127 if kind == "max" else 128)


def search_boards(positions):
    """Open positions of both movers, the empty board, and roots one move from a decided game (a win to take, a line to uncover)."""
    st, tm = positions
    open_ = np.flatnonzero(oracle.batch_winner(st) == 0)
    (sw, mw), (su, mu) = play(WIN_SEQ), play(UNCOVER_SEQ)
    st = np.concatenate([st[open_[:8]], np.array([sw, su], np.int8)])
    tm = np.concatenate([tm[open_[:8]], np.array([mw, mu], np.int8)])
    return np.ascontiguousarray(st), np.ascontiguousarray(tm)


@pytest.mark.parametrize("explore", [0, DEFAULT_EXPLORE, 1024])
@pytest.mark.parametrize("iterations", [1, 2, 3, 64, 512])
def test_search_equals_restatement(cpu, positions, iterations, explore):
    st, tm = search_boards(positions)
    if iterations == 512:  # (the restatement's walk is quadratic in the depth of the tree, and without an exploration term the tree
        # of an open board is one long line: an open board and the two decided roots, at explore 0 the decided roots alone)
        pick = [8, 9] if explore == 0 else [0, 8, 9]
        st, tm = st[pick], tm[pick]
    for hidden, kind in ((64, "random"), (256, "random"), (64, "zero"), (128, "mixed")):
        if iterations == 512 and hidden != 64:
            continue
        net = nets(hidden)[kind]
        same(run("tree_search_eval", "cpu", st, tm, None, (iterations, explore), net), R.restate_search(net, st, tm, None, iterations, explore))


def test_search_equals_restatement_with_masked_roots(cpu, positions):
    st, tm = search_boards(positions)
    legal = oracle.batch_legal_mask(st, tm)
    mask = (np.random.default_rng(6).random((len(st), 54)) < 0.4).astype(np.int8)
    mask[0] = 0  # no candidate
    mask[1] = 0
    mask[1, np.flatnonzero(legal[1])[3]] = 1  # one candidate
    mask[8] = 0
    mask[8, WIN_ACTION] = 1
    net = R.random_net(192, 2)
    got = run("tree_search_eval", "cpu", st, tm, mask, (48, DEFAULT_EXPLORE), net)
    same(got, R.restate_search(net, st, tm, mask, 48, DEFAULT_EXPLORE))
    v, w, l, a, nd, rv, rp = got.values()
    assert a[0] == -1 and nd[0] == 1 and not v[0].any() and not w[0].any() and not l[0].any() and not rp[0].any()
    assert rv[0] == R.restate_evaluate(net, st[:1], tm[:1])[1][0]  # the root's value is written all the same
    assert v[1].sum() == 48 and (v[1] > 0).sum() == 1 and rp[1].max() == 255
    assert a[8] == WIN_ACTION and w[8, WIN_ACTION] == 48 * 128 and nd[8] == 2


@pytest.fixture(scope="module")
def many():
    env = G.BatchedGobblet(120, "cpu", auto_reset=True, seed=11)
    env.rollout(29)
    st, tm = env.squares.numpy().copy(), env.to_move.numpy().copy()
    keep = oracle.batch_winner(st) == 0
    return st[keep], tm[keep]


def test_properties(cpu, many):
    st, tm = many
    n, I = len(st), 40
    net = R.random_net(128, 9)
    legal = oracle.batch_legal_mask(st, tm) != 0
    mask = (np.random.default_rng(8).random((n, 54)) < 0.5).astype(np.int8)
    mask[5] = 0
    got = run("tree_search_eval", "cpu", st, tm, mask, (I, DEFAULT_EXPLORE), net)
    v, w, l, a, nd, rv, rp = got.values()
    cand = legal & (mask != 0)
    has = cand.any(1)
    assert has.sum() > n - 5 and not has[5]
    assert (v.sum(1)[has] == I).all() and (v[~has] == 0).all()
    assert (v[~cand] == 0).all() and (w[~cand] == 0).all() and (l[~cand] == 0).all() and (rp[~cand] == 0).all() and (rp[cand] >= 1).all()
    assert (w >= 0).all() and (l >= 0).all() and ((w + l) <= v * 128).all()
    assert (nd <= I + 1).all() and (nd[has] >= 2).all() and (nd[~has] == 1).all() and (a[~has] == -1).all()
    assert (np.abs(rv) <= 128).all()
    same(run("tree_search_eval", "cpu", st, tm, mask, (I, DEFAULT_EXPLORE), net), got)  # two calls, one result
    for b in (0, 5, 17, n - 1):  # a board alone is the board in the batch
        alone = run("tree_search_eval", "cpu", st[b:b + 1], tm[b:b + 1], mask[b:b + 1], (I, DEFAULT_EXPLORE), net)
        same(alone, {k: x[b:b + 1] for k, x in got.items()})


def test_zero_evaluator_plays_the_immediate_win(cpu):
    """Uniform priors and value 0: the search still sees what the moves themselves decide.  The existing threat positions with the
    THREATENING side to move, and the decided-root boards: wherever the restatement finds the immediate win, so does the policy."""
    st, tm, _ = threat_positions(40, seed=100)
    (sw, mw), (su, mu) = play(WIN_SEQ), play(UNCOVER_SEQ)
    st = np.concatenate([st, np.array([sw, su], np.int8)])
    tm = np.concatenate([(1 - tm).astype(np.int8), np.array([mw, mu], np.int8)])
    net = R.zero_net(64)
    exp = R.restate_search(net, st, tm, None, 64, DEFAULT_EXPLORE)[3]
    found = [b for b in range(len(st)) if int(exp[b]) in winning_moves(st[b], int(tm[b]))]
    assert len(found) >= 35 and 40 in found
    pol = G.EvaluatorTreeSearchGobbletPolicy(G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, 0, 0, 0), iterations=64)
    a = pol.compute_actions_from_state(torch.from_numpy(st), torch.from_numpy(tm)).numpy()
    assert pol.explore == DEFAULT_EXPLORE and np.array_equal(a, exp)
    assert all(int(a[b]) in winning_moves(st[b], int(tm[b])) for b in found)
    assert a[40] == WIN_ACTION and a[41] != UNCOVER_ACTION


# ---- the recorded argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_replay_the_recorded_table(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "evaluator_arg_errors.json")))
    assert len(table) >= 40 and {c["fn"] for c in table} == {"evaluate", "tree_search_eval"}
    replay_arg_errors(table)
    for kw in ({"iterations": 0}, {"iterations": 513}, {"explore": -1}, {"explore": 1025}):
        with pytest.raises(ValueError):
            G.EvaluatorTreeSearchGobbletPolicy(G.GobbletEvaluator.from_float(*float_net(64, 1)), **kw)


# ---- the quantiser -------------------------------------------------------------------------------------------------------------------
def float_net(hidden, seed, grid=None):
    rng = np.random.default_rng(seed)
    if grid is None:
        return (rng.uniform(-1, 1, (117, hidden)), rng.uniform(-1, 1, hidden), rng.uniform(-1, 1, (hidden, 55)), rng.uniform(-1, 1, 55))
    return (rng.integers(-6, 7, (117, hidden)) / grid, rng.integers(-12, 5, hidden) / grid, rng.uniform(-1, 1, (hidden, 55)),
            rng.uniform(-1, 1, 55))


def test_from_float_returns_integer_weights_exactly():
    """Integer-valued weights over power-of-two scales come back as those integers (the largest magnitude 127 pins each scale)."""
    rng = np.random.default_rng(4)
    H = 128
    w1, w2 = rng.integers(-127, 128, (117, H)), rng.integers(-127, 128, (H, 56))
    w1[0, 0], w2[0, 0], w2[0, 54], w2[:, 55] = 127, -127, 127, 0
    b1, b2 = rng.integers(-5000, 5000, H), rng.integers(-(1 << 20), 1 << 20, 56)
    b2[55] = 0
    s1, hmax = 2.0 ** 5, 127 * 4 / 2.0 ** 5  # shift1 = 2: scale_h = 2^3
    sp, sv = 2.0 ** 2, 2.0 ** 6
    ev = G.GobbletEvaluator.from_float(w1 / s1, b1 / s1, np.concatenate([w2[:, :54] / sp, w2[:, 54:55] / sv], 1),
                                       np.concatenate([b2[:54] / (sp * 8), b2[54:55] / (sv * 8)]), hidden_max=hmax, natural_log=False)
    assert ev.scales == {"scale1": s1, "scale_h": 8.0, "scale_p": sp, "scale_v": sv, "fold": 1.0}
    assert (ev.shift1, ev.shift_p, ev.shift_v) == (2, 5, 2) and ev.hidden == H
    assert np.array_equal(ev.w1.numpy(), w1) and np.array_equal(ev.b1.numpy(), b1) and np.array_equal(ev.b2.numpy(), b2)
    assert np.array_equal(ev.w2.numpy(), R.Net(w1, b1, G.GobbletEvaluator.pack_w2(torch.from_numpy(w2)).numpy(), b2, 2, 5, 2).w2)
    assert np.array_equal(ev.w2.numpy().transpose(0, 2, 1).reshape(H, 56), w2)  # element [j // 4, k, j % 4] = weight j -> k


def test_from_float_keeps_the_policy_argmax(cpu, many):
    """Random float networks whose first layer lies on a grid the chosen scales represent exactly (the test asserts that the
    integer hidden units ARE the float ones times scale_h), so that what separates the integer logits from the float ones is the
    rounding of the second layer alone.  In units of one integer logit step (1/16 of an octave; the float logit times fold):
        |l_a - fold * logit_a| <= (sum_j h_j / 2 + 1/2) / 2^shift_p + 1
    -- every w2 entry is off by at most half a unit of scale_p, times its hidden unit; b2 by half a unit; the final shift floors.
    Two logits further apart than twice that bound cannot change places."""
    st, tm = many
    st, tm = st[:60], tm[:60]
    legal = oracle.batch_legal_mask(st, tm) != 0
    x = np.stack([np.asarray(oracle.observe(s, int(m), int(m))["observation"], np.float64).reshape(117) for s, m in zip(st, tm)])
    checked = 0
    for seed in range(3):
        w1, b1, w2, b2 = float_net(64, seed, grid=16)
        h = np.maximum(x @ w1 + b1, 0.0)
        ev = G.GobbletEvaluator.from_float(w1, b1, w2, b2, hidden_max=float(h.max()))
        sc = ev.scales
        hq = h * sc["scale_h"]
        assert np.array_equal(hq, np.rint(hq)) and hq.max() <= 127 and sc["scale_h"] >= 16  # layer 1 is exact
        step = (hq.sum(1) / 2 + 0.5) / 2.0 ** ev.shift_p + 1  # per board, in integer logit units
        logit = (h @ w2[:, :54] + b2[:54]) * sc["fold"]
        logit = np.where(legal, logit, -np.inf)
        top2 = np.sort(logit, 1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 2 * step
        pri, _ = ev.evaluate(torch.from_numpy(st), torch.from_numpy(tm))
        assert np.array_equal(pri.numpy().argmax(1)[clear], logit.argmax(1)[clear])
        assert np.allclose(pri.sum(1).numpy(), 1.0, atol=1e-6)
        checked += int(clear.sum())
    assert checked >= 60  # (of 180: the bound leaves enough positions to say something)


def test_policy_surface_on_cpu(cpu, many):
    st, tm = many
    st, tm = st[:30], tm[:30]
    net = R.random_net(64, 3)
    ev = G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, net.shift1, net.shift_p, net.shift_v)
    s = ev.as_struct()
    assert (s.hidden, s.shift1, s.w1) == (64, net.shift1, ev.w1.data_ptr()) and ev.to("cpu").w1.data_ptr() != ev.w1.data_ptr()
    pri, val = ev.evaluate(st, tm)
    exp_p, exp_v, _ = R.restate_evaluate(net, st, tm)
    assert pri.dtype == torch.float32 and np.allclose(pri.numpy(), exp_p / exp_p.sum(1, keepdims=True), rtol=1e-6, atol=0)
    assert np.array_equal(val.numpy(), (exp_v / 128.0).astype(np.float32))
    kw = dict(iterations=24, explore=96)
    exp = run("tree_search_eval", "cpu", st, tm, None, (24, 96), net)
    obs = torch.from_numpy(np.stack([oracle.observe(x, int(m), int(m))["observation"] for x, m in zip(st, tm)]))
    mask = torch.from_numpy(oracle.batch_legal_mask(st, tm))
    pol = G.EvaluatorTreeSearchGobbletPolicy(ev, **kw)
    a = pol.compute_actions(obs, mask)
    assert a.dtype == torch.int32 and np.array_equal(a.numpy(), exp["action"])
    vals = pol.action_values(st, tm)
    last = (pol.last_visits, pol.last_wins, pol.last_losses, pol.last_action, pol.last_nodes, pol.last_root_value, pol.last_root_priors)
    same(exp, [t.numpy() for t in last])
    seen = exp["visits"] > 0
    assert np.array_equal(vals.numpy()[seen], ((exp["wins"] - exp["losses"])[seen] / (exp["visits"][seen] * 128.0)).astype(np.float32))
    assert np.isneginf(vals.numpy()[~seen]).all()
    dist = pol.visit_distribution(st, tm)
    assert np.allclose(dist.numpy(), exp["visits"] / 24.0, rtol=1e-6, atol=0) and np.allclose(dist.sum(1).numpy(), 1.0)
    assert int(pol.compute_action(obs[0].numpy(), mask[0].numpy())) == int(exp["action"][0])
    r = pol.compute_actions_rllib({"observation": obs.numpy().reshape(30, -1), "action_mask": mask.numpy()})
    assert [int(x) for x in r] == exp["action"].tolist()
    f = pol.forward({"obs": {"obs": obs.numpy(), "mask": mask.numpy()}})
    assert f["act"].dtype == np.int64 and f["act"].tolist() == exp["action"].tolist()
    for bad in (dict(shift1=25), dict(shift_p=-1)):
        with pytest.raises(ValueError):
            G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, **{**dict(shift1=0, shift_p=0, shift_v=0), **bad})
    with pytest.raises(ValueError):
        G.GobbletEvaluator(net.w1, net.b1 + (1 << 21), net.w2, net.b2, 0, 0, 0)
