"""The device edges of k_playout, k_tree, k_collect_search and k_outcome_targets that the other GPU modules leave out (-m gpu):
ragged tiles, unroll remainders, NULL outputs and padded strides of the outcome targets against their definition; the per-board
tallies of gbl_collect_search against the recorded trajectory; the budgets the packed fields are sized for; more boards than the
grid cap (the grid-stride loop's second trip); canaries around every output, unaligned inputs and "non-zero" byte values.  Every
expected value is exact."""
import numpy as np
import pytest
import torch

import oracle
from tests import test_playout_policy as PP
from tests.search_harness import DEV, PLAYOUT_NAMES, G, midgame_boards, run, same  # noqa: F401  (G: the fixture)
from tests.search_harness import TREE_NAMES as NAMES
from tests.test_gpu_selfplay_search import device_collect
from tests.test_search_edges import (EXPLORES, I_MAX, M_MAX, PLAYOUT_BYTES, TREE_BYTES, byte_value_boards, check_saturated_collect,
                                     check_saturated_tree, saturated_boards, saturated_collect_args)
from tests.test_search_edges import CALL as SAT_CALL
from tests.test_search_edges import ENV_BASE as SAT_ENV_BASE
from tests.test_search_edges import SEED as SAT_SEED
from tests.test_selfplay_search import SCALARS, cells, collect, strides, targets_numpy
from tests.test_selfplay_search import same as same_collect
from tests.test_tree_policy import restate

pytestmark = pytest.mark.gpu

GRID_CAP = 1 << 20  # the kernels' largest grid: board b of a larger batch is served by workgroup b % 2^20 on its trip b / 2^20
TRAJ = [k for k, _, _ in SCALARS]


@pytest.fixture(scope="module")
def c5(G):
    return midgame_boards(turn=True)


def to(device, a):
    """A copy of `a` on `device` (a copy on the host too: the host flavour writes its in/out arguments in place)."""
    return torch.from_numpy(np.array(a)).to(device)


# ---- B1: k_outcome_targets against the definition --------------------------------------------------------------------------------
def device_targets(G, done, rewards, mover, layout, with_left=True):
    """The device twin of tests.test_selfplay_search.targets: padded strides, sentinel 77, nothing outside the cells written."""
    nat = G._native
    Tn, n = done.shape
    ps, ts, total = strides(n, Tn, layout)
    at = cells(n, Tn, layout)
    d, r, m = np.zeros(total, np.int8), np.zeros((total, 2), np.int8), np.zeros(total, np.int8)
    d[at], r[at], m[at] = done, rewards, mover
    d_d, d_r, d_m = to(DEV, d), to(DEV, r), to(DEV, m)
    z, left = to(DEV, np.full(total, 77, np.int8)), to(DEV, np.full(total, 77, np.int16))
    nat.check(nat.lib().gbl_outcome_targets(d_d.data_ptr(), d_r.data_ptr(), d_m.data_ptr(), z.data_ptr(), left.data_ptr() if with_left else None,
                                            n, ps, ts, Tn, nat.current_stream(DEV)), "gbl_outcome_targets")
    torch.cuda.synchronize()
    z, left = z.cpu().numpy(), left.cpu().numpy()
    untouched = np.ones(total, bool)
    untouched[at.ravel()] = False
    assert (z[untouched] == 77).all() and (left[untouched] == 77).all()  # (nothing outside the cells is written)
    assert with_left or (left == 77).all()
    assert np.array_equal(d_d.cpu().numpy(), d) and np.array_equal(d_r.cpu().numpy(), r) and np.array_equal(d_m.cpu().numpy(), m)  # inputs are inputs
    return z[at], left[at]


@pytest.mark.parametrize("layout", ["time", "tile"])
def test_outcome_targets_equal_the_definition(G, layout):
    """One lane, a ragged tile of 63, a full one, a second tile of one board, a third of two; every remainder of the four-ply unroll."""
    rng = np.random.default_rng(31)
    for n in (1, 63, 64, 65, 130):
        for Tn in (1, 2, 3, 5, 6, 7, 9):
            done = np.where(rng.random((Tn, n)) < 0.2, rng.choice(np.array([1, 1, -1, 2], np.int8), (Tn, n)), 0).astype(np.int8)  # non-zero = ended
            rewards = rng.integers(-1, 2, (Tn, n, 2)).astype(np.int8)  # (also where no game ends: a reward there is not an outcome)
            mover = rng.integers(0, 2, (Tn, n)).astype(np.int8)
            ez, el = targets_numpy(done, rewards, mover)
            z, left = device_targets(G, done, rewards, mover, layout)
            assert np.array_equal(z, ez) and np.array_equal(left, el), (n, Tn, np.argwhere(z != ez)[:5], np.argwhere(left != el)[:5])
            z0, _ = device_targets(G, done, rewards, mover, layout, with_left=False)  # plies_left_traj = NULL: z unchanged
            assert np.array_equal(z0, ez), (n, Tn)


@pytest.mark.parametrize("layout", ["time", "tile"])
def test_outcome_targets_hand_made_ends(G, layout):
    """The pattern of tests.test_selfplay_search.test_outcome_targets with its literal expectations: an end on the first ply, on the
    last ply, none, two in the window, an illegal-terminate end (mover -1, other 0)."""
    nat = G._native
    Tn, n = 6, 70
    done, rewards = np.zeros((Tn, n), np.int8), np.zeros((Tn, n, 2), np.int8)
    mover = ((np.arange(Tn)[:, None] + np.arange(n)) % 2).astype(np.int8)
    done[0, 0], rewards[0, 0] = 1, (1, -1)
    done[Tn - 1, 1], rewards[Tn - 1, 1] = 1, (-1, 1)
    done[1, 3], rewards[1, 3] = 1, (-1, 1)
    done[4, 3], rewards[4, 3] = 1, (1, -1)
    done[2, 65], rewards[2, 65] = 1, (0, -1)
    rewards[3, 2] = (1, -1)  # a reward without a game end is not an outcome
    z, left = device_targets(G, done, rewards, mover, layout)
    ez, el = targets_numpy(done, rewards, mover)
    assert np.array_equal(z, ez) and np.array_equal(left, el)
    assert (z[:, 2] == nat.Z_OPEN).all() and (left[:, 2] == -1).all() and (z[1:, 0] == nat.Z_OPEN).all() and left[0, 0] == 0
    assert (left[:, 1] == np.arange(Tn)[::-1]).all() and list(left[:, 3]) == [1, 0, 2, 1, 0, -1]
    assert set(z[:3, 65].tolist()) == {0, -1} and z[0, 3] == rewards[1, 3, mover[0, 3]]
    assert np.array_equal(device_targets(G, done, rewards, mover, layout, with_left=False)[0], ez)


@pytest.mark.parametrize("layout", ["time", "tile"])
def test_outcome_targets_at_the_ply_limit(G, layout):
    """plies = 32767 (the argument's limit, plies_left up to 32766 in an int16), one game end: the last ply of board 0."""
    nat = G._native
    Tn, n = 32767, 65
    rng = np.random.default_rng(32)
    done = np.zeros((Tn, n), np.int8)
    done[Tn - 1, 0] = 1
    rewards = rng.integers(-1, 2, (Tn, n, 2)).astype(np.int8)
    rewards[Tn - 1, 0] = (1, -1)
    mover = rng.integers(0, 2, (Tn, n)).astype(np.int8)
    ez, el = np.full((Tn, n), nat.Z_OPEN, np.int8), np.full((Tn, n), -1, np.int16)
    el[:, 0] = Tn - 1 - np.arange(Tn)  # (the definition in closed form: targets_numpy is quadratic in the plies)
    ez[:, 0] = np.where(mover[:, 0] != 0, -1, 1)
    z, left = device_targets(G, done, rewards, mover, layout)
    assert np.array_equal(z, ez) and np.array_equal(left, el)
    assert left[0, 0] == 32766 and left[Tn - 1, 0] == 0


# ---- B2: gbl_collect_search's tallies and NULL outputs ----------------------------------------------------------------------------
def tallies_of(tr, n, T):
    """What the four tallies of a launch must be, from its recorded trajectory."""
    return [n * T, int((tr["done"] != 0).sum()), int((tr["winner"] == 1).sum()), int((tr["winner"] == -1).sum())]


@pytest.mark.parametrize("n", [1, 65, 257, 4099])
def test_collect_search_tallies_and_two_outputs(G, c5, n):
    """Only winner_traj and done_traj given, and the counters: the call of tests.test_selfplay_search.test_tallies_and_null_outputs."""
    nat = G._native
    st, tm, turn = c5[0][:n], c5[1][:n], c5[2][:n] % 9
    T = 6
    finished = 0
    for layout in ("time", "tile"):
        for pols in (("tree", "random"), ("tree", "tree")):
            args = (T, pols, (16, 12), (4, 3), 30, 64, 2, nat.ILLEGAL_NOOP, layout, 3, 17, 4)
            host = collect(nat.cpu_raw(), st, tm, turn, *args)
            full = device_collect(G, st, tm, turn, *args)
            same_collect(full, host)
            counters = torch.zeros((nat.COUNTER_STRIPES, nat.COUNTER_STRIDE), dtype=torch.int64, device=DEV)
            some = device_collect(G, st, tm, turn, *args, keep=("winner", "done"), counters=counters)
            assert set(some[0]) == {"winner", "done"}
            for k in some[0]:
                assert np.array_equal(some[0][k], full[0][k]) and np.array_equal(some[0][k], host[0][k]), (layout, pols, k)
            for name, g, e in zip(("state", "to_move", "done", "turn"), some[1:], host[1:]):
                assert np.array_equal(g, e), (layout, pols, name)
            c = counters.cpu().numpy()
            first = tallies_of(some[0], n, T)
            assert c.sum(0)[:4].tolist() == first and not c[:, 4:].any(), (layout, pols, c.sum(0), first)
            # a second launch on the same counters (another seed: other games) adds its own tallies
            args2 = args[:-3] + (4, 17, 4)
            again = device_collect(G, st, tm, turn, *args2, keep=("winner", "done"), counters=counters)
            second = tallies_of(again[0], n, T)
            assert counters.cpu().numpy().sum(0)[:4].tolist() == [a + b for a, b in zip(first, second)], (layout, pols)
            finished += first[1] + second[1]
    assert finished > 0 or n < 257  # (the searching side finishes games inside six plies)


def test_collect_search_each_output_null_in_turn(G, c5):
    nat = G._native
    n = 257
    st, tm, turn = c5[0][:n], c5[1][:n], c5[2][:n] % 9
    args = (5, ("tree", "tree"), (16, 12), (4, 3), 30, 64, 3, nat.ILLEGAL_TERMINATE, "tile", 3, 17, 4)
    full = device_collect(G, st, tm, turn, *args)
    for missing in TRAJ:
        keep = [k for k in TRAJ if k != missing]
        got = device_collect(G, st, tm, turn, *args, keep=keep)
        assert set(got[0]) == set(keep)
        for k in keep:
            assert np.array_equal(got[0][k], full[0][k]), (missing, k)
        for name, g, e in zip(("state", "to_move", "done", "turn"), got[1:], full[1:]):
            assert np.array_equal(g, e), (missing, name)


def test_python_surface_counts_like_the_host_flavour(G):
    kw = dict(iterations=16, playouts=4, max_plies=30, explore=64)
    delta, games = {}, {}
    for device in (DEV, "cpu"):
        env = G.BatchedGobblet(257, device, auto_reset=True, seed=4, env_base=3, track_turn=True)
        env.rollout(9, count=True)
        before = env.counters.cpu().clone()
        out = env.collect(6, policies=("tree", "random"), search=kw, count=True)
        delta[device] = (env.counters.cpu() - before).tolist()
        games[device] = [257 * 6, int((out["done"] != 0).sum()), int((out["winner"] == 1).sum()), int((out["winner"] == -1).sum())]
    assert delta[DEV] == delta["cpu"] == games[DEV] == games["cpu"]
    assert delta[DEV][1] > 0


# ---- B3: the budgets the packed fields are sized for ------------------------------------------------------------------------------
@pytest.mark.parametrize("playouts", [256, 130, 63])  # three boards: k_tree<4>, <2>, <1>
def test_saturated_tree_equals_restatement(G, playouts):
    st, tm, mask, _ = saturated_boards()
    assert G._native.lib() is not None
    for explore in EXPLORES:
        got = run("tree_search", DEV, st, tm, mask, (I_MAX, playouts, M_MAX, explore, SAT_SEED, SAT_ENV_BASE, SAT_CALL))
        check_saturated_tree(got, explore, playouts)


@pytest.mark.parametrize("sample_plies", [0, 1])
def test_saturated_collect_equals_restatement(G, sample_plies):
    for layout in ("time", "tile"):
        check_saturated_collect(device_collect(G, *saturated_collect_args(sample_plies, layout)), sample_plies)


def test_saturated_open_children_equal_host_flavour(G, c5):
    """Two candidates per board: two children of about 512 visits of 256 games each, all of them played (the restatement is out of
    reach here; the host flavour is tied to it at these operands by tests/test_search_edges.py)."""
    st, tm = c5[0][:4], c5[1][:4]
    rng = np.random.default_rng(33)
    legal = oracle.batch_legal_mask(st, tm)
    mask = np.zeros((4, 54), np.int8)
    for b in range(4):
        mask[b, rng.choice(np.flatnonzero(legal[b]), 2, replace=False)] = 1
    args = (I_MAX, 256, M_MAX, 16, 2, SAT_ENV_BASE - 1, SAT_CALL)
    got = run("tree_search", DEV, st, tm, mask, args)
    same(got, run("tree_search", "cpu", st, tm, mask, args))
    v, w, l = got["visits"], got["wins"], got["losses"]
    assert ((v > 0).sum(1) == 2).all() and (v.sum(1) == I_MAX).all() and (w + l <= v * 256).all() and (w + l).sum() > 4 * 128 * 256
    pargs = (4096, M_MAX, 2, SAT_ENV_BASE - 1, SAT_CALL)
    gotp = run("playout_values", DEV, st, tm, mask, pargs)
    same(gotp, run("playout_values", "cpu", st, tm, mask, pargs))
    assert ((gotp["wins"] + gotp["losses"]) <= 4096).all() and (gotp["wins"] + gotp["losses"]).sum() > 4 * 4096


# ---- B4: more boards than the grid cap --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def beyond(c5):
    """2^20 + 65 boards: the grid-stride loops' second trip runs on 65 workgroups."""
    n = GRID_CAP + 65
    st, tm = np.resize(c5[0], (n, 27)), np.resize(c5[1], n)
    assert np.array_equal(st[65536:131072], c5[0]) and np.array_equal(st[GRID_CAP:], c5[0][:65])
    return st, tm


def check_beyond(name, beyond, params, keep):
    """Whole arrays against the host flavour, and the second trip's boards against a launch of their own at env_base + 2^20
    (a second trip that keeps anything of the first -- its tree's links, its counters, its board ids -- differs from it)."""
    st, tm = beyond
    seed_at = {"tree_search": 4, "playout_values": 2}[name]  # (params: ..., seed, env_base, call)
    assert params[seed_at + 1] == 5
    got = run(name, DEV, st, tm, None, params, keep=keep)
    assert set(got) == set(keep)
    same(got, run(name, "cpu", st, tm, None, params, keep=keep))
    tail_params = params[:seed_at + 1] + (5 + GRID_CAP,) + params[seed_at + 2:]
    tail = run(name, DEV, st[GRID_CAP:], tm[GRID_CAP:], None, tail_params)
    for k in keep:
        assert np.array_equal(got[k][GRID_CAP:], tail[k]), k
    return got


def test_tree_search_beyond_the_grid_cap(G, beyond):
    got = check_beyond("tree_search", beyond, (2, 1, 2, 16, 7, 5, 3), ("visits", "action", "nodes", "plies"))
    assert (got["visits"].sum(1) == 2).all() and (got["nodes"] >= 2).all() and (got["nodes"] <= 3).all()


def test_playout_values_beyond_the_grid_cap(G, beyond):
    got = check_beyond("playout_values", beyond, (1, 2, 7, 5, 3), ("wins", "action", "plies"))
    assert (got["wins"] >= 0).all() and (got["wins"] <= 1).all()


def test_collect_search_beyond_the_grid_cap(G, beyond):
    nat = G._native
    st, tm = beyond
    args = (2, ("tree", "random"), (2, 2), (1, 1), 2, 16, 0, nat.ILLEGAL_NOOP, "time", 7, 5, 3)
    keep = ("actions", "done")
    got = device_collect(G, st, tm, None, *args, keep=keep)
    exp = collect(nat.cpu_raw(), st, tm, None, *args, keep=keep)
    tail = device_collect(G, st[GRID_CAP:], tm[GRID_CAP:], None, *args[:-2], 5 + GRID_CAP, 3, keep=keep)
    for k in keep:
        assert np.array_equal(got[0][k], exp[0][k]), (k, np.argwhere(got[0][k] != exp[0][k])[:5])
        assert np.array_equal(got[0][k][:, GRID_CAP:], tail[0][k]), k
    for name, g, e, t in zip(("state", "to_move", "done"), got[1:4], exp[1:4], tail[1:4]):
        assert np.array_equal(g, e) and np.array_equal(g[GRID_CAP:], t), name


# ---- B5: canaries, unaligned inputs, byte values --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257])
def test_search_outputs_stay_inside_their_arrays(G, c5, n):
    st, tm = np.array(c5[0][:n]), np.array(c5[1][:n])
    mask = (np.random.default_rng(n).random((n, 54)) < 0.5).astype(np.int8)
    targs = (40, 6, 30, 64, 3, 17, 4)
    same(run("tree_search", DEV, st, tm, mask, targs, misaligned=True), run("tree_search", DEV, st, tm, mask, targs))
    pargs = (8, 30, 3, 17, 4)
    same(run("playout_values", DEV, st, tm, mask, pargs, misaligned=True), run("playout_values", DEV, st, tm, mask, pargs))


def test_each_search_output_null_in_turn(G, c5):
    n = 65
    st, tm = c5[0][:n], c5[1][:n]
    mask = (np.random.default_rng(n).random((n, 54)) < 0.5).astype(np.int8)
    for name, names, params in (("tree_search", NAMES, (40, 6, 30, 64, 3, 17, 4)), ("playout_values", PLAYOUT_NAMES, (8, 30, 3, 17, 4))):
        full = run(name, DEV, st, tm, mask, params)
        for missing in names:
            keep = [k for k in names if k != missing]
            got = run(name, DEV, st, tm, mask, params, keep=keep)
            assert set(got) == set(keep)
            same(got, full)


def test_nonzero_bytes_are_set_bytes_on_the_device(G):
    """to_move and mask bytes of -128, -1, 2 and 127 are read as set: the 0 / 1 inputs' result, which is the restatement's."""
    st, tm, mask, tm2, mask2 = byte_value_boards()
    exp = restate(st, tm, mask, *TREE_BYTES)
    same(run("tree_search", DEV, st, tm, mask, TREE_BYTES), exp)
    same(run("tree_search", DEV, st, tm2, mask2, TREE_BYTES), exp)
    exp = PP.restate(st, tm, mask, *PLAYOUT_BYTES)
    same(run("playout_values", DEV, st, tm, mask, PLAYOUT_BYTES), exp)
    same(run("playout_values", DEV, st, tm2, mask2, PLAYOUT_BYTES), exp)
