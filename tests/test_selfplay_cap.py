"""Playout-cap randomisation on the host flavour (no GPU): gbl_cpu_collect_search_cap against the restatement of the header text
(tests/cap_restatement.py: the draw on the oracle's Philox, the window composed of gbl_cpu_solve, gbl_cpu_tree_search_eval_noise and
gbl_cpu_step_into), the draw pinned by numbers, the identities the contract states, the consumers downstream, shards and *ply_dev, the
argument errors of both flavours in their order, and the Python surface on device="cpu"."""
import ctypes as C

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import cap_restatement as CR
from tests import evaluator_restatement as R
from tests.search_harness import run
from tests.selfplay_cap_harness import FULL, host_collect_cap
from tests.selfplay_harness import _evaluator, call_args, same
from tests.test_selfplay_solve import EXPLORE, collect_solve, fixture_boards, smoke_net

N_BOARDS, T = 130, 6
ITS, FAST, SHARE = (8, 5), (3, 1), (128, 64)  # both sides capped, differently
SEED = 7


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def nets():
    return smoke_net(), R.random_net(128, 77)  # H = 64 and 128


@pytest.fixture(scope="module")
def boards():
    """130 boards: 40 empty ones (the whole opening inside the sampled plies) and 90 of the midgame fixture."""
    st, tm, turn = fixture_boards(N_BOARDS - 40)
    return (np.ascontiguousarray(np.concatenate([np.zeros((40, 27), np.int8), st])), np.concatenate([np.zeros(40, np.int8), tm]),
            np.concatenate([np.zeros(40, np.int32), turn % 6]).astype(np.int32))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deps,noise,sample_plies", [((0, 0), (0, 0), 0), ((3, 3), (64, 64), 4), ((0, 3), (64, 0), 4), ((3, 0), (0, 64), 0)])
def test_window_equals_composed_loop(cpu, nets, boards, deps, noise, sample_plies):
    st, tm, turn = boards
    plies, s, tn, roots = CR.composed_loop(cpu, st, tm, turn, T, ("eval", "eval"), nets, ITS, FAST, SHARE, deps, noise, EXPLORE, sample_plies,
                                           SEED, 0, 8)
    for layout, ply_dev in (("time", None), ("tile", 3)):
        got = host_collect_cap(st, tm, turn, T, ("eval", "eval"), nets, ITS, FAST, SHARE, deps, noise, EXPLORE, sample_plies, layout=layout,
                               seed=SEED, ply0=8 - (ply_dev or 0), ply_dev=ply_dev)
        for t, ply in enumerate(plies):
            for k, v in ply.items():
                assert got[0][k].dtype == v.dtype and np.array_equal(got[0][k][t], v), (layout, t, k)
        assert np.array_equal(got[1], s) and np.array_equal(got[4], tn)
    tr = got[0]
    how, mover = tr["how"], tr["mover"]
    for m in (0, 1):  # every shape holds both kinds of ply on both sides
        assert ((how == nat.HOW_SEARCH) & (mover == m)).any() and ((how == nat.HOW_FAST) & (mover == m)).any()
    if sample_plies:
        assert (how == nat.HOW_FAST_SAMPLED).any() and (how == nat.HOW_SEARCH_SAMPLED).any()
    if any(deps):
        assert (how == nat.HOW_PROVEN).any()
    fast = (how == nat.HOW_FAST) | (how == nat.HOW_FAST_SAMPLED)
    assert not tr["visits"][fast].any() and (tr["nodes"][fast] >= 1).all() and tr["priors"][fast].any()
    assert ((tr["visits"].sum(-1) > 0) == np.isin(how, (nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED, nat.HOW_PROVEN))).all()
    # 3c. a fast ply's nodes, value, root_value and priors are gbl_cpu_tree_search_eval's at fast_iterations over the same candidates
    checked = 0
    for t, b in np.argwhere(fast)[::7]:
        m = int(mover[t, b])
        mask = (tr["outcomes"][t, b] == 0).astype(np.int8)[None] if deps[m] else None
        rs, rm = roots[t][0][b:b + 1], roots[t][1][b:b + 1]
        exp = run("tree_search_eval", "cpu", rs, rm, mask, (FAST[m], EXPLORE), nets[m])
        assert tr["nodes"][t, b] == exp["nodes"][0] and tr["root_value"][t, b] == exp["root_value"][0]
        assert tr["value"][t, b] == (exp["wins"][0] - exp["losses"][0]).sum() and np.array_equal(tr["priors"][t, b], exp["root_priors"][0])
        if how[t, b] == nat.HOW_FAST:
            assert tr["actions"][t, b] == exp["action"][0]
        checked += 1
    assert checked >= 20


# ---- 2. the draw, pinned independently of the code under test -----------------------------------------------------------------------
PINNED = {7: (99, (16, 16, 17, 14, 22, 14)), 1: (95, (18, 15, 17, 19, 12, 14))}  # seed -> full draws of boards 0 .. 64 x plies 0 .. 5 at share 64


def test_the_draw_is_pinned(cpu, nets):
    ids, plies = torch.arange(65), torch.arange(6)
    assert G.cap_full(7, torch.tensor([0]), plies, 0.5).tolist() == [False, True, False, True, False, False]  # share 128, board 0
    assert [q for q in range(6) if CR.is_full(7, 0, q, 128)] == [1, 3]
    for seed, (total, per_ply) in PINNED.items():
        got = G.cap_full(seed, ids[None, :], plies[:, None], 0.25)
        assert got.dtype == torch.bool and tuple(got.shape) == (6, 65)
        assert int(got.sum()) == total and tuple(got.sum(1).tolist()) == per_ply
        assert np.array_equal(got.numpy(), CR.full_table(seed, range(65), range(6), 64))
        # the `how` bytes of an unguarded window from the empty position
        st, tm, turn = np.zeros((65, 27), np.int8), np.zeros(65, np.int8), np.zeros(65, np.int32)
        how = host_collect_cap(st, tm, turn, 6, ("eval", "eval"), nets, ITS, FAST, (64, 64), noise=(64, 64), X=EXPLORE, seed=seed,
                               keep=("how",))[0]["how"]
        assert np.array_equal(how == nat.HOW_SEARCH, got.numpy()) and np.array_equal(how == nat.HOW_FAST, ~got.numpy())
    assert bool(G.cap_full(3, ids, 5, 1.0).all()) and not bool(G.cap_full(3, ids, 5, 0.0).any())
    big = G.cap_full(2 ** 64 - 1, torch.tensor([(1 << 42) - 1]), (1 << 24) - 1, 0.5)
    assert bool(big[0]) == CR.is_full(2 ** 64 - 1, (1 << 42) - 1, (1 << 24) - 1, 128)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            G.cap_full(1, ids, 0, bad)


# ---- 3. the identities ----------------------------------------------------------------------------------------------------------------
def test_identities(cpu, nets, boards):
    st, tm, turn = boards
    for deps, noise, sp in (((3, 0), (64, 32), 4), ((0, 0), (0, 0), 0)):
        args = (st, tm, turn, T, ("eval", "eval"), nets, ITS, deps, EXPLORE, sp, nat.ILLEGAL_NOOP, "tile", SEED, 5, 2)
        plain = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, *args, noise=noise)
        # shares (256, 256): gbl_cpu_collect_search_noise on every array; the fast budgets are not read there
        got = host_collect_cap(st, tm, turn, T, ("eval", "eval"), nets, ITS, (-3, 999), (FULL, FULL), deps, noise, EXPLORE, sp, layout="tile",
                               seed=SEED, env_base=5, ply0=2)
        same(got, plain)
    # share 0 with fast = iterations and no noise: gbl_cpu_collect_search_solve but for `how` and the visits of the searched plies
    deps, sp = (3, 2), 4
    args = (st, tm, turn, T, ("eval", "eval"), nets, ITS, deps, EXPLORE, sp, nat.ILLEGAL_NOOP, "time", SEED, 5, 2)
    plain = collect_solve(cpu.gbl_cpu_collect_search_solve, cpu.gbl_cpu_last_error, *args)
    got = host_collect_cap(st, tm, turn, T, ("eval", "eval"), nets, ITS, ITS, (0, 0), deps, (0, 0), EXPLORE, sp, seed=SEED, env_base=5, ply0=2)
    for k in plain[0]:
        if k not in ("how", "visits"):
            assert np.array_equal(got[0][k], plain[0][k]), k
    hp, hg = plain[0]["how"], got[0]["how"]
    moved = {nat.HOW_SEARCH: nat.HOW_FAST, nat.HOW_SEARCH_SAMPLED: nat.HOW_FAST_SAMPLED, nat.HOW_PROVEN: nat.HOW_PROVEN}
    assert set(np.unique(hp)) == set(moved) and all(np.array_equal(hg == v, hp == k) for k, v in moved.items())
    hot = hp == nat.HOW_PROVEN
    assert np.array_equal(got[0]["visits"][hot], plain[0]["visits"][hot]) and not got[0]["visits"][~hot].any()
    for x, y in zip(got[1:], plain[1:]):
        assert np.array_equal(x, y)
    # a RANDOM side reads neither parameter
    pols, use = ("random", "eval"), (None, nets[1])
    a = host_collect_cap(st, tm, turn, T, pols, use, (0, 5), (0, 2), (FULL, 64), seed=SEED)
    b = host_collect_cap(st, tm, turn, T, pols, use, (0, 5), (77, 2), (-9, 64), seed=SEED)
    same(a, b)
    assert (a[0]["how"] == nat.HOW_RANDOM).any() and (a[0]["how"] == nat.HOW_FAST).any()


# ---- 4. downstream unchanged ----------------------------------------------------------------------------------------------------------
def test_outcome_targets_and_replay_take_the_window_as_it_is(cpu, nets):
    n = 130
    ev = tuple(_evaluator(x) for x in nets)
    env = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=11, track_turn=True)
    env.rollout(40)
    tr = env.collect(T, policies=("evaluator", "evaluator"), out="fresh",
                     search=dict(evaluator=ev, iterations=ITS, explore=EXPLORE, solve_depth=(2, 0), noise=0.25, sample_plies=44,
                                 cap=dict(fast_iterations=FAST, full=(0.5, 0.25))))
    env.outcome_targets(tr)
    how, z, done = tr["how"].numpy(), tr["z"].numpy(), tr["done"].numpy()
    assert (how >= nat.HOW_FAST).any() and np.isin(how, (3, 4, 5, 8, 9)).all()
    keep = np.zeros_like(how, bool)
    keep[1:] = (z[1:] != nat.Z_OPEN) & (done[:-1] == 0) & np.isin(how[1:], (nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED, nat.HOW_PROVEN))
    dropped = np.zeros_like(keep)
    dropped[1:] = (z[1:] != nat.Z_OPEN) & (done[:-1] == 0) & (how[1:] >= nat.HOW_FAST)
    K = int(keep.sum())
    assert K > 50 and dropped.sum() > 50  # (the fast plies are what the window loses)
    buf = G.ReplayBuffer(1024, "cpu")
    buf.append(env, tr, tag=3)
    assert buf.total == K and int(buf._state[1]) == K
    at = np.argwhere(keep)  # ascending (t, b)
    tt, bb = at[:, 0], at[:, 1]
    assert np.array_equal(buf.visits[:K].numpy(), tr["visits"].numpy()[tt, bb])
    assert np.array_equal(buf.action_mask[:K].numpy(), tr["action_mask"].numpy()[tt - 1, bb])
    assert np.array_equal(buf.observation[:K].numpy(), tr["observation"].numpy().reshape(T, n, 117)[tt - 1, bb])
    assert np.array_equal(buf.z[:K].numpy(), z[tt, bb]) and np.array_equal(buf.mover[:K].numpy(), tr["mover"].numpy()[tt, bb])
    assert (buf.tag[:K] == 3).all() and not buf.visits[K:].any()
    drawn = buf.batch(512, symmetries=None, call=1, seed=5)
    slot = drawn["index"][:, 0].numpy()
    assert (slot >= 0).all() and (slot < K).all() and len(set(slot.tolist())) > K // 2
    assert np.isin(how[tt[slot], bb[slot]], (3, 4, 5)).all() and (drawn["visits"].numpy().sum(1) > 0).all()
    assert np.array_equal(drawn["visits"].numpy(), tr["visits"].numpy()[tt[slot], bb[slot]])
    # gbl_training_batch draws from the same cells
    tb = env.training_batch(tr, 256, symmetries=None, call=2)
    t_, b_ = tb["index"][:, 0].numpy(), tb["index"][:, 1].numpy()
    ok = t_ >= 0
    assert ok.sum() > 128 and keep[t_[ok], b_[ok]].all()


# ---- 5. shards and *ply_dev -------------------------------------------------------------------------------------------------------------
def test_shards_and_ply_dev(cpu, nets, boards):
    st, tm, turn = boards
    kw = dict(deps=(3, 0), noise=(64, 64), X=EXPLORE, sample_plies=4, seed=SEED)
    whole = host_collect_cap(st, tm, turn, T, ("eval", "eval"), nets, ITS, FAST, SHARE, ply0=3, **kw)
    halves = [host_collect_cap(st[a:b], tm[a:b], turn[a:b], T, ("eval", "eval"), nets, ITS, FAST, SHARE, env_base=a, ply0=3, **kw)
              for a, b in ((0, 65), (65, 130))]
    for k, v in whole[0].items():
        assert np.array_equal(v, np.concatenate([h[0][k] for h in halves], axis=1)), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(whole[i], np.concatenate([h[i] for h in halves]))
    same(host_collect_cap(st, tm, turn, T, ("eval", "eval"), nets, ITS, FAST, SHARE, ply0=0, ply_dev=3, **kw), whole)
    other = host_collect_cap(st, tm, turn, T, ("eval", "eval"), nets, ITS, FAST, SHARE, ply0=4, **kw)
    assert not np.array_equal(other[0]["how"], whole[0]["how"])  # (the draw moves with the ply index)


# ---- 6. the argument errors, in the stated order ----------------------------------------------------------------------------------------
SHARE_MSG = b"full_share0 / full_share1 must be in [0, 256]"
FAST_MSG = b"fast_iterations0 / fast_iterations1 must be in [1, iterations]"
NOISE_MSG = b"noise0 / noise1 must be in [0, 256]"
CASES = [  # (name, overrides, message or None: GBL_OK)
    ("share -1", dict(share=(-1, 64)), SHARE_MSG),
    ("share 257", dict(share=(64, 257)), SHARE_MSG),
    ("fast 0", dict(fast=(0, 1)), FAST_MSG),
    ("fast > iterations", dict(fast=(3, 6)), FAST_MSG),
    ("the noise check comes first", dict(noise=(300, 0), share=(-1, 64)), NOISE_MSG),
    ("an earlier check comes first", dict(deps=(9, 0), share=(-1, 64), fast=(0, 0)), b"solve_depth0 / solve_depth1 must be in [0, 6]"),
    ("the shares come before the budgets", dict(share=(0, 999), fast=(0, 1)), SHARE_MSG),
    ("a RANDOM side reads neither", dict(pols=("random", "eval"), share=(-5, 64), fast=(99, 1)), None),
    ("a RANDOM side's budget is not read", dict(pols=("eval", "random"), share=(0, 0), fast=(8, 0)), None),
    ("fast is not read at share 256", dict(share=(256, 64), fast=(-1, 5)), None),
    ("the ends of the ranges", dict(share=(0, 256), fast=(8, 0)), None),
    ("fast = iterations, fast = 1", dict(share=(0, 255), fast=(8, 1)), None),
]


@pytest.mark.parametrize("flavour", ["host", "device"])
def test_argument_errors(flavour):
    lib, prefix = (nat.cpu_raw(), "gbl_cpu_") if flavour == "host" else (nat.lib(), "gbl_")
    f, err = getattr(lib, prefix + "collect_search_cap"), getattr(lib, prefix + "last_error")
    net = smoke_net()
    for name, over, msg in CASES:
        kw = dict(pols=("eval", "eval"), its=(8, 5), deps=(0, 0), noise=(0, 0), fast=(3, 1), share=(64, 64))
        kw.update(over)
        evs = [net.struct() if p == "eval" else None for p in kw["pols"]]
        # n = 0: every check of the arguments runs, and nothing is read or launched
        rc = f(*call_args("cap", lambda a: a, None, None, None, {}, 0, 64, 64, 1, 0, 0, None, 4, kw["pols"], 16, 0, nat.ILLEGAL_NOOP, None, None,
                          None, evs=evs, its=kw["its"], deps=kw["deps"], noise=kw["noise"], fast=kw["fast"], share=kw["share"]))
        if msg is None:
            assert rc == nat.OK, (name, err())
        else:
            assert rc == nat.ERR_ARG and err() == msg, (name, rc, err())


# ---- the Python surface on device="cpu" -------------------------------------------------------------------------------------------------
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


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "observation", "done")


def _collect(n, policies, search, seed=11, **kw):
    env = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, env_base=3, track_turn=True)
    env.rollout(30)
    env._lib = Counting(env._lib)
    return env.collect(4, policies=policies, search=search, out="fresh", **kw), env


def test_collect_cap(cpu, nets):
    net = nets[0]
    ev = _evaluator(net)
    base = dict(evaluator=ev, iterations=8, sample_plies=32, explore=24, noise=0.25)
    plain, env0 = _collect(40, ("evaluator", "evaluator"), dict(base))
    assert set(env0._lib.calls) == {"gbl_collect_search_noise"}  # no cap: today's entry point
    for full in (1, 1.0, (1, 1.0)):  # full = 1 keeps it too
        one, env1 = _collect(40, ("evaluator", "evaluator"), dict(base, cap=dict(fast_iterations=2, full=full)))
        assert set(env1._lib.calls) == {"gbl_collect_search_noise"} and all(torch.equal(one[k], plain[k]) for k in KEYS)
    capped, env2 = _collect(40, ("evaluator", "evaluator"), dict(base, cap=dict(fast_iterations=(3, 2), full=(0.5, 0.25))))
    assert set(env2._lib.calls) == {"gbl_collect_search_cap"}
    ref = G.BatchedGobblet(40, "cpu", auto_reset=True, seed=11, env_base=3, track_turn=True)
    ref.rollout(30)
    raw = host_collect_cap(ref.squares.numpy(), ref.to_move.numpy(), ref.turn.numpy(), 4, ("eval", "eval"), (net, net), (8, 8), (3, 2), (128, 64),
                           noise=(64, 64), X=24, sample_plies=32, seed=11, env_base=3, ply0=30)[0]
    for k in ("actions", "visits", "value", "nodes", "how", "root_value", "priors"):
        assert np.array_equal(capped[k].numpy(), raw[k]), k
    how = capped["how"].numpy()
    assert (how >= nat.HOW_FAST).any() and (how <= nat.HOW_SEARCH_SAMPLED).any()
    # G.cap_full recomputes the draws (no guard: every ply takes one)
    ids, q = 3 + torch.arange(40), 30 + torch.arange(4)
    full = torch.where(capped["mover"] == 0, G.cap_full(11, ids[None, :], q[:, None], 0.5), G.cap_full(11, ids[None, :], q[:, None], 0.25))
    assert torch.equal(full, capped["how"] <= nat.HOW_SEARCH_SAMPLED)
    # the defaults; with the guard; one side capped; a random side's values are dropped
    d, env3 = _collect(40, ("evaluator", "evaluator"), dict(base, iterations=32, cap={}))
    assert set(env3._lib.calls) == {"gbl_collect_search_cap"} and 0.1 < float((d["how"] <= 4).float().mean()) < 0.45
    g, env4 = _collect(40, ("evaluator", "evaluator"), dict(base, solve_depth=(2, 3), cap=dict(fast_iterations=2, full=0.25)))
    assert set(env4._lib.calls) == {"gbl_collect_search_cap"} and "outcomes" in g and (g["how"] == nat.HOW_PROVEN).any()
    r, env5 = _collect(40, ("random", "evaluator"), dict(base, cap=dict(fast_iterations=(99, 2), full=(0.0, 1.0))))
    assert set(env5._lib.calls) == {"gbl_collect_search_noise"}
    r, env6 = _collect(40, ("random", "evaluator"), dict(base, cap=dict(fast_iterations=(99, 2), full=(1.0, 0.0))))
    assert set(env6._lib.calls) == {"gbl_collect_search_cap"} and set(np.unique(r["how"].numpy())) <= {0, 8, 9}
    for bad in (dict(full=-0.5), dict(full=2), dict(full=(0.1, 0.2, 0.3)), dict(fast_iterations=0), dict(fast_iterations=9),
                dict(fast_iterations=(1, 2, 3)), dict(fast=3), 0.25, (16, 0.25)):
        with pytest.raises(ValueError):
            _collect(8, ("evaluator", "evaluator"), dict(base, cap=bad))
    with pytest.raises(ValueError):  # no evaluator side: the key is unknown
        _collect(8, ("tree", "tree"), dict(iterations=8, playouts=2, cap=dict(full=0.5)))


def test_cap_does_not_go_with_the_tablebase(cpu, nets):
    ev = _evaluator(nets[0])
    tb = G.Tablebase((1, 0, 0), "cpu")
    tb.build()
    cap = dict(fast_iterations=2, full=0.25)
    env = G.BatchedGobblet(8, "cpu", auto_reset=True, seed=1, track_turn=True)
    with pytest.raises(ValueError, match="cap"):
        env.collect(3, policies=("tablebase", "evaluator"), search=dict(tablebase=tb, evaluator=ev, iterations=8, cap=cap))
    with pytest.raises(ValueError, match="cap"):
        env.collect(3, policies=("evaluator", "evaluator"), search=dict(tablebase=tb, judge=True, evaluator=ev, iterations=8, cap=cap))
    with pytest.raises(ValueError, match="cap"):
        env.collect(3, policies=("tablebase", "random"), search=dict(tablebase=tb, cap=cap))
