"""Root noise on the host flavour (no GPU): gbl_cpu_tree_search_eval_noise and gbl_cpu_collect_search_noise against the restatement of
the header text (tests/noise_restatement.py) -- the noise row, the mix, the search, the self-play loop -- plus the identities the
contract states (w = 0, explore = 0, a board alone, a shard), the diversity the noise is there for, the recorded argument errors of
both flavours and the Python surface on device="cpu"."""
import json
import os

import numpy as np
import pytest
import torch

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests import noise_restatement as N
from tests import solver_restatement as SR
from tests.search_harness import SEARCH_NAMES, replay_arg_errors, run
from tests.search_harness import same as same_arrays
from tests.selfplay_harness import _evaluator, same
from tests.test_playout_policy import random_midgames
from tests.test_selfplay_solve import EXPLORE, collect_solve, fixture_boards, smoke_net

SEED, ENV_BASE = 0xFEDCBA9876543210, (1 << 41) + 77


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def midgames():
    st, tm = random_midgames(6, seed=21, max_plies=20)
    return np.ascontiguousarray(st), np.ascontiguousarray(tm)


# ---- the row rule and the mix ----------------------------------------------------------------------------------------------------------
ROW_CALLS = (0, 1, 2, 3, 1000, 65535, (1 << 24) - 2, (1 << 24) - 1)  # 8 calls x 512 boards = 4 096 (g, q) pairs


def row_masks(size, n, rng):
    """n candidate sets of `size` actions of the empty board (every action is legal there)."""
    mask = np.zeros((n, 54), np.int8)
    for b in range(n):
        mask[b, rng.choice(54, size, replace=False)] = 1
    return mask


@pytest.mark.parametrize("size", [1, 2, 9, 27, 54])
def test_noise_row_equals_restatement(cpu, size):
    n = 512
    st, tm = np.zeros((n, 27), np.int8), np.zeros(n, np.int8)
    net = R.zero_net(64)
    mask = row_masks(size, n, np.random.default_rng(size))
    for i, q in enumerate(ROW_CALLS):
        base = ENV_BASE if i & 1 else i * 1000
        nu = run("tree_search_eval_noise", "cpu", st, tm, mask, (1, 0, 256, SEED, base, q), net)["root_mixed"]  # (w = 256: pi' is nu itself)
        exp = np.stack([N.noise_row(SEED, base + b, q, mask[b] != 0) for b in range(n)])
        assert np.array_equal(nu, exp), (size, q)
        total = nu.astype(np.int64).sum(1)
        assert (total >= 255).all() and (total <= 254 + size).all()  # (the floor loses less than one per candidate)
        assert (nu[mask == 0] == 0).all() and (nu[mask != 0] >= 1).all()
        if size == 1:
            assert (nu[mask != 0] == 255).all()
    assert len({nu[b].tobytes() for b in range(n)}) > (1 if size == 1 else n // 2)  # (the rows differ from board to board)


@pytest.mark.parametrize("w", [1, 64, 128, 255, 256])
def test_mix_equals_restatement(cpu, midgames, w):
    st, tm = midgames
    for hidden in (64, 256):
        net = R.random_net(hidden, 5 + hidden)
        got = run("tree_search_eval_noise", "cpu", st, tm, None, (1, EXPLORE, w, SEED, ENV_BASE, 9), net)
        pi = R.restate_evaluate(net, st, tm)[0]
        assert np.array_equal(got["root_priors"], pi)  # root_priors_out stays the network's row
        for b in range(len(st)):
            cand = oracle.legal_mask(st[b], int(tm[b])) != 0
            nu = N.noise_row(SEED, ENV_BASE + b, 9, cand)
            assert np.array_equal(got["root_mixed"][b], N.mix(pi[b], nu, w, cand)), (w, b)
            if w == 256:
                assert np.array_equal(got["root_mixed"][b], nu)


def test_mix_stays_a_prior_byte():
    """(pi (256 - w) + nu w + 128) >> 8 over all prior bytes and weights stays in 1 .. 255: exhaustive."""
    pi, nu, w = np.meshgrid(np.arange(1, 256), np.arange(1, 256), np.arange(0, 257), indexing="ij")
    out = (pi * (256 - w) + nu * w + 128) >> 8
    assert out.min() == 1 and out.max() == 255


# ---- the search ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 8, 64])
@pytest.mark.parametrize("hidden", [64, 256])
def test_search_equals_restatement(cpu, midgames, hidden, iterations):
    st, tm = midgames
    net = R.random_net(hidden, 5 + hidden)
    legal = oracle.batch_legal_mask(st, tm)
    mask = np.ones((len(st), 54), np.int8)
    mask[0] = 0  # no candidate: nothing is searched, nothing is drawn
    mask[1] = 0
    mask[1, np.flatnonzero(legal[1])[3]] = 1  # one candidate
    for w, msk in ((64, None), (256, None), (128, mask)):
        params = (iterations, EXPLORE, w, SEED, ENV_BASE, 5)
        got = run("tree_search_eval_noise", "cpu", st, tm, msk, params, net)
        same_arrays(got, N.restate_search_noise(net, st, tm, msk, *params))
    v, w_, l, a, nd, rv, rp, rm = got.values()
    assert a[0] == -1 and nd[0] == 1 and not v[0].any() and not rp[0].any() and not rm[0].any()
    assert v[1].sum() == iterations and rp[1].max() == 255 and rm[1].max() == 255 and (rm[1] > 0).sum() == 1


def test_identities(cpu):
    st, tm, _ = fixture_boards(40)
    net = smoke_net()
    I = 24
    plain = run("tree_search_eval", "cpu", st, tm, None, (I, EXPLORE), net)
    # w = 0 is gbl_cpu_tree_search_eval on every shared output, and root_mixed_out is the network's row
    got = run("tree_search_eval_noise", "cpu", st, tm, None, (I, EXPLORE, 0, SEED, ENV_BASE, 3), net)
    same_arrays(plain, got)
    assert np.array_equal(got["root_mixed"], plain["root_priors"])
    # explore = 0: the prior never enters the key, so only root_mixed_out differs
    flat = run("tree_search_eval", "cpu", st, tm, None, (I, 0), net)
    got0 = run("tree_search_eval_noise", "cpu", st, tm, None, (I, 0, 200, SEED, ENV_BASE, 3), net)
    same_arrays(flat, got0)
    assert not np.array_equal(got0["root_mixed"], flat["root_priors"])
    # the noise changes what the search looks at
    noisy = run("tree_search_eval_noise", "cpu", st, tm, None, (I, EXPLORE, 128, SEED, ENV_BASE, 3), net)
    assert np.array_equal(noisy["root_priors"], plain["root_priors"]) and np.array_equal(noisy["root_value"], plain["root_value"])
    assert not np.array_equal(noisy["visits"], plain["visits"])
    # NULL for root_mixed_out (and every output is optional, as in gbl_tree_search_eval)
    same_arrays(run("tree_search_eval_noise", "cpu", st, tm, None, (I, EXPLORE, 128, SEED, ENV_BASE, 3), net, keep=SEARCH_NAMES), noisy)
    # a board alone is the board in the batch; board k + b of a batch at env_base 0 is board b of the shard at env_base k
    for b in (0, 7, 39):
        alone = run("tree_search_eval_noise", "cpu", st[b:b + 1], tm[b:b + 1], None, (I, EXPLORE, 128, SEED, ENV_BASE + b, 3), net)
        same_arrays(alone, {k: x[b:b + 1] for k, x in noisy.items()})
    whole = run("tree_search_eval_noise", "cpu", st, tm, None, (I, EXPLORE, 128, SEED, 0, 3), net)
    shard = run("tree_search_eval_noise", "cpu", st[16:], tm[16:], None, (I, EXPLORE, 128, SEED, 16, 3), net)
    same_arrays(shard, {k: x[16:] for k, x in whole.items()})
    # the call index and the seed both move the row
    other = run("tree_search_eval_noise", "cpu", st, tm, None, (I, EXPLORE, 128, SEED, ENV_BASE, 4), net)
    assert not np.array_equal(other["root_mixed"], noisy["root_mixed"])
    other = run("tree_search_eval_noise", "cpu", st, tm, None, (I, EXPLORE, 128, SEED + 1, ENV_BASE, 3), net)
    assert not np.array_equal(other["root_mixed"], noisy["root_mixed"])


# ---- self-play ----------------------------------------------------------------------------------------------------------------------------
def five_boards():
    st, tm, turn = fixture_boards(4)
    return (np.concatenate([np.zeros((1, 27), np.int8), st]), np.concatenate([np.zeros(1, np.int8), tm]),
            np.concatenate([np.zeros(1, np.int32), turn % 3]))


def composed_loop(cpu, st, tm, turn, T, nets, its, deps, noise, X, sample_plies, seed, env_base, ply0):
    """gbl_cpu_solve -> gbl_cpu_tree_search_eval_noise(mask = C, call = q) -> the stream-4 draw -> gbl_cpu_step_into, ply by ply."""
    from tests.test_selfplay_search import STREAM_VISIT, visits_draw
    n = len(st)
    s, m, d, tn = st.copy(), tm.copy(), np.zeros(n, np.int8), turn.astype(np.int32).copy()
    plies = []
    for t in range(T):
        q = ply0 + t
        act, vis, val, nod = np.zeros(n, np.int32), np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32)
        rv, pri, how = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8), np.zeros(n, np.int8)
        outcome, proven = np.full((n, 54), SR.NONE, np.int8), np.zeros(n, np.int8)
        for b in range(n):
            mv = int(m[b])
            mask = None
            if deps[mv] > 0:
                o, V, a_star = run("solve", "cpu", s[b:b + 1], m[b:b + 1], None, (deps[mv],)).values()
                outcome[b], proven[b] = o[0], V[0]
                if V[0] != 0:
                    act[b], how[b], vis[b, a_star[0]] = a_star[0], nat.HOW_PROVEN, its[mv]
                    val[b] = (1 if V[0] > 0 else -1) * 128 * its[mv]
                    continue
                mask = (o == 0).astype(np.int8)
            v, w, l, a, nd, rq, rp, _ = run("tree_search_eval_noise", "cpu", s[b:b + 1], m[b:b + 1], mask,
                                            (its[mv], X, noise[mv], seed, env_base + b, q), nets[mv]).values()
            vis[b], val[b], nod[b], rv[b], pri[b] = v[0], (w[0] - l[0]).sum(), nd[0], rq[0], rp[0]
            if tn[b] < sample_plies:
                act[b], how[b] = visits_draw(v[0], N.word(seed, env_base + b, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
            else:
                act[b], how[b] = a[0], nat.HOW_SEARCH
        mover = m.copy()
        win, rew = np.zeros(n, np.int8), np.zeros((n, 2), np.int8)
        mask_, obs = np.zeros((n, 54), np.int8), np.zeros((n, 117), np.int8)
        rc = cpu.gbl_cpu_step_into(s.ctypes.data, m.ctypes.data, d.ctypes.data, act.ctypes.data, win.ctypes.data, rew.ctypes.data,
                                   mask_.ctypes.data, obs.ctypes.data, tn.ctypes.data, None, None, None, n, nat.ILLEGAL_NOOP, 1, None)
        assert rc == 0, cpu.gbl_cpu_last_error()
        plies.append(dict(actions=act, visits=vis, value=val, nodes=nod, root_value=rv, priors=pri, how=how, outcomes=outcome, proven=proven,
                          mover=mover, winner=win, rewards=rew, done=d.copy(), to_move=m.copy(), action_mask=mask_, observation=obs))
    return plies, s, tn


@pytest.mark.parametrize("noise", [(64, 0), (64, 256)])
@pytest.mark.parametrize("deps", [(0, 0), (2, 0)])
@pytest.mark.parametrize("sample_plies", [0, 2])
def test_selfplay_equals_composed_loop_and_restatement(cpu, sample_plies, deps, noise):
    st, tm, turn = five_boards()
    nets, its, T = (smoke_net(), R.random_net(128, 77)), (8, 5), 6
    plies, s, tn = composed_loop(cpu, st, tm, turn, T, nets, its, deps, noise, EXPLORE, sample_plies, 9, ENV_BASE, 8)
    for layout, ply_dev in (("time", None), ("tile", 3)):
        got = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, st, tm, turn, T, ("eval", "eval"), nets, its, deps,
                            EXPLORE, sample_plies, nat.ILLEGAL_NOOP, layout, 9, ENV_BASE, 8 - (ply_dev or 0), ply_dev, noise=noise)
        for t, ply in enumerate(plies):
            for k, v in ply.items():
                assert np.array_equal(got[0][k][t], v), (layout, t, k)
        assert np.array_equal(got[1], s) and np.array_equal(got[4], tn)
    tr = got[0]
    assert ((tr["how"] == nat.HOW_PROVEN) == (tr["proven"] != 0)).all()
    hot = tr["how"] == nat.HOW_PROVEN
    assert ((tr["visits"][hot] > 0).sum(1) == 1).all() and not tr["priors"][hot].any()
    if sample_plies == 0 and deps == (2, 0):  # once more against the oracle's loop (the restatement of the whole contract)
        exp = N.restate_collect_noise(st, tm, turn, T, ("eval", "eval"), nets, its, deps, noise, EXPLORE, 0, nat.ILLEGAL_NOOP, 9, ENV_BASE, 8)
        same(got, exp)


def test_selfplay_identities(cpu):
    st, tm, turn = fixture_boards(20)
    turn = turn % 4
    net = smoke_net()
    for pols, its, deps in ((("eval", "eval"), (8, 3), (2, 3)), (("eval", "eval"), (8, 3), (0, 0)), (("random", "eval"), (0, 5), (0, 2))):
        use = tuple(net if p == "eval" else None for p in pols)
        args = (st, tm, turn, 4, pols, use, its, deps, EXPLORE, 2, nat.ILLEGAL_TERMINATE, "tile", 3, 17, 4)
        plain = collect_solve(cpu.gbl_cpu_collect_search_solve, cpu.gbl_cpu_last_error, *args)
        # weights (0, 0): gbl_cpu_collect_search_solve on every array
        same(collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, *args, noise=(0, 0)), plain)
        if pols[0] == "random":  # a RANDOM side ignores its weight, whatever it is
            a = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, *args, noise=(0, 64))
            b = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, *args, noise=(999, 64))
            same(a, b)
            assert not np.array_equal(a[0]["visits"], plain[0]["visits"])


DIVERSE_NET_SEED, DIVERSE_SEQUENCES = 0, 10  # the first R.random_net(64, seed) for which the RESTATEMENT plays >= 8 sequences, and how many


def test_noise_makes_the_games_differ(cpu):
    """64 boards from the empty position, one network, 8 plies, no sampled plies.  Without noise the search draws nothing, so every
    board plays the same game; with weight 64 on both sides the restatement (N.restate_collect_noise, run once when this test was
    written: 10 sequences with network seed 0, the first seed with at least 8) says how many different games there are."""
    n, T = 64, 8
    st, tm, turn = np.zeros((n, 27), np.int8), np.zeros(n, np.int8), np.zeros(n, np.int32)
    net = R.random_net(64, DIVERSE_NET_SEED)
    args = (st, tm, turn, T, ("eval", "eval"), (net, net), (8, 8), (0, 0), 16, 0, nat.ILLEGAL_NOOP, "time", 1, 0, 0)
    plain = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, *args, noise=(0, 0))[0]["actions"].T
    assert len({tuple(r) for r in plain}) == 1
    noisy = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, *args, noise=(64, 64))[0]["actions"].T
    assert len({tuple(r) for r in noisy}) == DIVERSE_SEQUENCES >= 8
    k = 12  # the first boards once more against the restatement itself (a board's game depends on its id alone)
    exp = N.restate_collect_noise(st[:k], tm[:k], turn[:k], T, ("eval", "eval"), (net, net), (8, 8), (0, 0), (64, 64), 16, 0, nat.ILLEGAL_NOOP,
                                  1, 0, 0)[0]["actions"].T
    assert np.array_equal(noisy[:k], exp)


# ---- the recorded argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors_replay_the_recorded_table(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "noise_arg_errors.json")))
    assert len(table) >= 20 and {c["fn"] for c in table} == {"tree_search_eval_noise", "collect_search_noise"}
    replay_arg_errors(table)


# ---- the Python surface on device="cpu" ----------------------------------------------------------------------------------------------------
class Counting:
    """A library handle that counts the calls of every entry point it hands out."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


def test_policy_noise(cpu):
    st, tm, _ = fixture_boards(30)
    net = smoke_net()
    ev = _evaluator(net)
    pol = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=16, explore=EXPLORE, noise=0.25, seed=5, env_base=100)
    assert pol.noise == 64 and pol.call == 0
    pol._lib = Counting(pol._lib)
    for call in range(2):  # `call` counts up once per compute_actions_from_state
        a = pol.compute_actions_from_state(torch.from_numpy(st), torch.from_numpy(tm)).numpy()
        exp = run("tree_search_eval_noise", "cpu", st, tm, None, (16, EXPLORE, 64, 5, 100, call), net)
        assert np.array_equal(a, exp["action"]) and np.array_equal(pol.last_visits.numpy(), exp["visits"])
        assert np.array_equal(pol.last_root_priors.numpy(), exp["root_priors"]) and np.array_equal(pol.last_root_mixed.numpy(), exp["root_mixed"])
        assert pol.call == call + 1
        # G.root_noise rebuilds the row the root kept from the network's row
        nu = G.root_noise(5, 100 + np.arange(30), call, oracle.batch_legal_mask(st, tm))
        assert nu.dtype == torch.uint8 and tuple(nu.shape) == (30, 54)
        pi = pol.last_root_priors.to(torch.int64)
        mixed = torch.where(pi > 0, (pi * (256 - 64) + nu.to(torch.int64) * 64 + 128) >> 8, torch.zeros_like(pi))
        assert torch.equal(mixed.to(torch.uint8), pol.last_root_mixed)
    assert pol._lib.calls == {"gbl_tree_search_eval_noise": 2}
    quiet = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=16, explore=EXPLORE)  # noise 0: exactly what it called before
    quiet._lib = Counting(quiet._lib)
    a = quiet.compute_actions_from_state(torch.from_numpy(st), torch.from_numpy(tm)).numpy()
    assert quiet._lib.calls == {"gbl_tree_search_eval": 1} and quiet.call == 0
    assert np.array_equal(a, run("tree_search_eval", "cpu", st, tm, None, (16, EXPLORE), net)["action"])
    assert quiet.last_root_mixed is quiet.last_root_priors
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            G.EvaluatorTreeSearchGobbletPolicy(ev, noise=bad)


def test_root_noise_equals_root_mixed_out(cpu):
    """G.root_noise against root_mixed_out at w = 256 (nu itself), byte for byte: large board ids, the last call index, masks."""
    n = 200
    st, tm = np.zeros((n, 27), np.int8), np.zeros(n, np.int8)
    mask = (np.random.default_rng(2).random((n, 54)) < 0.3).astype(np.int8)
    mask[3] = 0
    for seed, base, q in ((SEED, ENV_BASE, (1 << 24) - 1), (1, 0, 0), (2 ** 64 - 1, (1 << 42) - n, 77)):
        exp = run("tree_search_eval_noise", "cpu", st, tm, mask, (1, 0, 256, seed, base, q), R.zero_net(64))["root_mixed"]
        got = G.root_noise(seed, base + np.arange(n), q, torch.from_numpy(mask))
        assert np.array_equal(got.numpy(), exp)
    per_board = G.root_noise(1, np.arange(n), np.arange(n) % 5, mask)  # a ply per board
    for q in range(5):
        rows = np.flatnonzero(np.arange(n) % 5 == q)
        assert np.array_equal(per_board.numpy()[rows], G.root_noise(1, rows, q, mask[rows]).numpy())


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "observation", "done")


def _collect(n, policies, search, seed=11, **kw):
    env = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, env_base=3, track_turn=True)
    env.rollout(30)
    env._lib = Counting(env._lib)
    return env.collect(4, policies=policies, search=search, out="fresh", **kw), env


def test_collect_noise(cpu):
    net = smoke_net()
    ev = _evaluator(net)
    base = dict(evaluator=ev, iterations=8, sample_plies=40, explore=24)
    plain, env0 = _collect(40, ("evaluator", "evaluator"), dict(base))
    assert set(env0._lib.calls) == {"gbl_collect_search_eval"}  # no noise: the old entry point
    zero, env1 = _collect(40, ("evaluator", "evaluator"), dict(base, noise=0))
    assert set(env1._lib.calls) == {"gbl_collect_search_eval"} and all(torch.equal(zero[k], plain[k]) for k in KEYS)
    guard, env2 = _collect(40, ("evaluator", "evaluator"), dict(base, solve_depth=2, noise=(0.0, 0)))
    assert set(env2._lib.calls) == {"gbl_collect_search_solve"}
    # a value: both sides; against the raw entry point on the same boards
    both, env3 = _collect(40, ("evaluator", "evaluator"), dict(base, noise=0.25))
    assert set(env3._lib.calls) == {"gbl_collect_search_noise"} and not torch.equal(both["visits"], plain["visits"])
    ref = G.BatchedGobblet(40, "cpu", auto_reset=True, seed=11, env_base=3, track_turn=True)
    ref.rollout(30)
    raw = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, ref.squares.numpy(), ref.to_move.numpy(),
                        ref.turn.numpy(), 4, ("eval", "eval"), (net, net), (8, 8), (0, 0), 24, 40, nat.ILLEGAL_NOOP, "time", 11, 3, 30,
                        noise=(64, 64))[0]
    for k in ("actions", "visits", "value", "nodes", "how", "root_value", "priors"):
        assert np.array_equal(both[k].numpy(), raw[k]), k
    # a pair: one side only (an arena noises one side, or none)
    one, _ = _collect(40, ("evaluator", "evaluator"), dict(base, noise=(0.25, 0)))
    mover = one["mover"].numpy()
    assert np.array_equal(one["visits"].numpy()[0][mover[0] == 1], plain["visits"].numpy()[0][mover[0] == 1])
    assert not torch.equal(one["visits"], plain["visits"]) and not torch.equal(one["visits"], both["visits"])
    # a policy instance as a side contributes its own noise
    inst = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=8, explore=24, noise=0.25)
    mixed, env4 = _collect(40, (inst, "evaluator"), dict(evaluator=ev, iterations=8, sample_plies=40))
    assert set(env4._lib.calls) == {"gbl_collect_search_noise"} and all(torch.equal(mixed[k], one[k]) for k in KEYS)
    # with the guard: the solver's arrays come too, proven plies draw nothing
    g, env5 = _collect(40, ("evaluator", "evaluator"), dict(base, solve_depth=(2, 3), noise=0.5))
    assert set(env5._lib.calls) == {"gbl_collect_search_noise"} and "outcomes" in g and (g["how"] == nat.HOW_PROVEN).any()
    # the noise on a RANDOM side is dropped; a bad share is refused
    r, env6 = _collect(40, ("random", "evaluator"), dict(base, noise=(1.0, 0)))
    assert set(env6._lib.calls) == {"gbl_collect_search_eval"}
    for bad in (-0.5, 2, (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError):
            _collect(8, ("evaluator", "evaluator"), dict(base, noise=bad))
