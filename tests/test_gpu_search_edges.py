"""The device edges of k_playout, k_tree, k_collect_search and k_outcome_targets that the other GPU modules leave out (-m gpu):
ragged tiles, unroll remainders, NULL outputs and padded strides of the outcome targets against their definition; the per-board
tallies of gbl_collect_search against the recorded trajectory; the budgets the packed fields are sized for; more boards than the
grid cap (the grid-stride loop's second trip); canaries around every output, unaligned inputs and "non-zero" byte values.  Every
expected value is exact."""
import numpy as np
import pytest
import torch

import oracle
from tests import test_gpu_playout_policy as GP
from tests import test_playout_policy as PP
from tests.test_gpu_selfplay_search import device_collect
from tests.test_gpu_tree_policy import device_run, same
from tests.test_search_edges import (EXPLORES, I_MAX, M_MAX, PLAYOUT_BYTES, TREE_BYTES, byte_value_boards, check_saturated_collect,
                                     check_saturated_tree, saturated_boards, saturated_collect_args)
from tests.test_search_edges import CALL as SAT_CALL
from tests.test_search_edges import ENV_BASE as SAT_ENV_BASE
from tests.test_search_edges import SEED as SAT_SEED
from tests.test_selfplay_search import CODES, SCALARS, cells, collect, strides, targets_numpy
from tests.test_selfplay_search import same as same_collect
from tests.test_tree_policy import NAMES, restate, run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
THREADS = 16
GRID_CAP = 1 << 20  # the kernels' largest grid: board b of a larger batch is served by workgroup b % 2^20 on its trip b / 2^20
PLAYOUT_NAMES = ("wins", "losses", "action", "plies")
TRAJ = [k for k, _, _ in SCALARS]


@pytest.fixture(scope="module")
def G():
    import gobblet_rl_amd as g
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    g._native.lib()
    g._native.cpu_raw().gbl_cpu_set_threads(THREADS)
    return g


@pytest.fixture(scope="module")
def c5(G):
    """The 65 536 midgame boards of the other GPU modules, with their turn counters."""
    env = G.BatchedGobblet(65536, DEV, auto_reset=True, seed=11, track_turn=True)
    env.rollout(64)
    torch.cuda.synchronize()
    st, tm, turn = env.squares.cpu().numpy().copy(), env.to_move.cpu().numpy().copy(), env.turn.cpu().numpy().copy()
    assert (oracle.batch_winner(st) == 0).all() and 0.3 < tm.mean() < 0.7
    return st, tm, turn


def to(device, a):
    """A copy of `a` on `device` (a copy on the host too: the host flavour writes its in/out arguments in place)."""
    return torch.from_numpy(np.array(a)).to(device)


def entry(G, device, name):
    """(entry point, stream) of gbl_<name> for the device flavour or, with device "cpu", the host flavour."""
    nat = G._native
    if device == "cpu":
        return getattr(nat.cpu_raw(), "gbl_cpu_" + name), None
    return getattr(nat.lib(), "gbl_" + name), nat.current_stream(device)


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
def collect_some(G, device, st, tm, turn, T, pols, its, pls, M, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, keep=TRAJ,
                 counters=None):
    """gbl_collect_search of either flavour with only the trajectory arrays named in `keep` given (the others NULL), and optionally
    tallies.  Returns ({name: (T, n, ...)}, state, to_move, done, turn) like tests.test_selfplay_search.collect."""
    nat = G._native
    f, stream = entry(G, device, "collect_search")
    n = len(st)
    ps, ts, total = strides(n, T, layout)
    traj = {k: to(device, np.full((total,) + tail, -7, dt)) for k, dt, tail in SCALARS if k in keep}
    d_st, d_tm, d_dn = to(device, np.asarray(st, np.int8)), to(device, np.asarray(tm, np.int8)), to(device, np.full(n, 5, np.int8))
    d_tn = None if turn is None else to(device, np.asarray(turn, np.int32))
    rc = f(d_st.data_ptr(), d_tm.data_ptr(), d_dn.data_ptr(), *[nat.ptr(traj.get(k)) for k in TRAJ], n, ps, ts, seed, env_base, ply0, None, T,
           CODES[pols[0]], CODES[pols[1]], its[0], its[1], pls[0], pls[1], M, X, sample_plies, illegal_mode, nat.ptr(counters), nat.ptr(d_tn), stream)
    assert rc == 0, (nat.lib().gbl_last_error(), nat.cpu_raw().gbl_cpu_last_error())
    if device != "cpu":
        torch.cuda.synchronize()
    at = cells(n, T, layout)
    untouched = np.ones(total, bool)
    untouched[at.ravel()] = False
    host = {k: v.cpu().numpy() for k, v in traj.items()}
    assert all((v[untouched] == -7).all() for v in host.values())  # (nothing outside the cells is written)
    return ({k: v[at] for k, v in host.items()}, d_st.cpu().numpy(), d_tm.cpu().numpy(), d_dn.cpu().numpy(), None if d_tn is None else d_tn.cpu().numpy())


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
            some = collect_some(G, DEV, st, tm, turn, *args, keep=("winner", "done"), counters=counters)
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
            again = collect_some(G, DEV, st, tm, turn, *args2, keep=("winner", "done"), counters=counters)
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
        got = collect_some(G, DEV, st, tm, turn, *args, keep=keep)
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
        got = device_run(G, st, tm, mask, I_MAX, playouts, M_MAX, explore, SAT_SEED, SAT_ENV_BASE, SAT_CALL)
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
    cpu = G._native.cpu_raw()
    args = (I_MAX, 256, M_MAX, 16, 2, SAT_ENV_BASE - 1, SAT_CALL)
    got = device_run(G, st, tm, mask, *args)
    same(got, run(cpu, st, tm, mask, *args))
    v, w, l = got[:3]
    assert ((v > 0).sum(1) == 2).all() and (v.sum(1) == I_MAX).all() and (w + l <= v * 256).all() and (w + l).sum() > 4 * 128 * 256
    pargs = (4096, M_MAX, 2, SAT_ENV_BASE - 1, SAT_CALL)
    gotp = GP.device_run(G, st, tm, mask, *pargs)
    GP.same(gotp, PP.run(cpu, st, tm, mask, *pargs))
    assert ((gotp[0] + gotp[1]) <= 4096).all() and (gotp[0] + gotp[1]).sum() > 4 * 4096


# ---- B4: more boards than the grid cap --------------------------------------------------------------------------------------------
def search_some(G, device, name, names, st, tm, mask, params, keep):
    """gbl_tree_search / gbl_playout_values of either flavour with only the outputs named in `keep` given: {name: array}."""
    nat = G._native
    f, stream = entry(G, device, name)
    n = len(st)
    out = {k: torch.full((n, 54) if k in ("visits", "wins", "losses") else (n,), -7, dtype=torch.int32, device=device) for k in names if k in keep}
    d_st, d_tm, d_mk = to(device, st), to(device, tm), None if mask is None else to(device, mask)
    rc = f(d_st.data_ptr(), d_tm.data_ptr(), nat.ptr(d_mk), *params, *[nat.ptr(out.get(k)) for k in names], n, stream)
    assert rc == 0, (nat.lib().gbl_last_error(), nat.cpu_raw().gbl_cpu_last_error())
    if device != "cpu":
        torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def beyond(c5):
    """2^20 + 65 boards: the grid-stride loops' second trip runs on 65 workgroups."""
    n = GRID_CAP + 65
    st, tm = np.resize(c5[0], (n, 27)), np.resize(c5[1], n)
    assert np.array_equal(st[65536:131072], c5[0]) and np.array_equal(st[GRID_CAP:], c5[0][:65])
    return st, tm


def check_beyond(G, name, names, beyond, params, keep):
    """Whole arrays against the host flavour, and the second trip's boards against a launch of their own at env_base + 2^20
    (a second trip that keeps anything of the first -- its tree's links, its counters, its board ids -- differs from it)."""
    st, tm = beyond
    seed_at = {"tree_search": 4, "playout_values": 2}[name]  # (params: ..., seed, env_base, call)
    assert params[seed_at + 1] == 5
    got = search_some(G, DEV, name, names, st, tm, None, params, keep)
    exp = search_some(G, "cpu", name, names, st, tm, None, params, keep)
    assert set(got) == set(keep)
    for k in keep:
        assert np.array_equal(got[k], exp[k]), (k, np.argwhere(got[k] != exp[k])[:5])
    tail_params = params[:seed_at + 1] + (5 + GRID_CAP,) + params[seed_at + 2:]
    tail = search_some(G, DEV, name, names, st[GRID_CAP:], tm[GRID_CAP:], None, tail_params, names)
    for k in keep:
        assert np.array_equal(got[k][GRID_CAP:], tail[k]), k
    return got


def test_tree_search_beyond_the_grid_cap(G, beyond):
    got = check_beyond(G, "tree_search", NAMES, beyond, (2, 1, 2, 16, 7, 5, 3), ("visits", "action", "nodes", "plies"))
    assert (got["visits"].sum(1) == 2).all() and (got["nodes"] >= 2).all() and (got["nodes"] <= 3).all()


def test_playout_values_beyond_the_grid_cap(G, beyond):
    got = check_beyond(G, "playout_values", PLAYOUT_NAMES, beyond, (1, 2, 7, 5, 3), ("wins", "action", "plies"))
    assert (got["wins"] >= 0).all() and (got["wins"] <= 1).all()


def test_collect_search_beyond_the_grid_cap(G, beyond):
    nat = G._native
    st, tm = beyond
    args = (2, ("tree", "random"), (2, 2), (1, 1), 2, 16, 0, nat.ILLEGAL_NOOP, "time", 7, 5, 3)
    keep = ("actions", "done")
    got = collect_some(G, DEV, st, tm, None, *args, keep=keep)
    exp = collect_some(G, "cpu", st, tm, None, *args, keep=keep)
    tail = collect_some(G, DEV, st[GRID_CAP:], tm[GRID_CAP:], None, *args[:-2], 5 + GRID_CAP, 3, keep=keep)
    for k in keep:
        assert np.array_equal(got[0][k], exp[0][k]), (k, np.argwhere(got[0][k] != exp[0][k])[:5])
        assert np.array_equal(got[0][k][:, GRID_CAP:], tail[0][k]), k
    for name, g, e, t in zip(("state", "to_move", "done"), got[1:4], exp[1:4], tail[1:4]):
        assert np.array_equal(g, e) and np.array_equal(g[GRID_CAP:], t), name


# ---- B5: canaries, unaligned inputs, byte values --------------------------------------------------------------------------------------
GUARD = 0x5A


def guarded(device_bytes_before, array):
    """`array` copied into a guard-filled device buffer, `device_bytes_before` bytes in; (the view, the whole buffer as bytes)."""
    raw = np.ascontiguousarray(array).view(np.uint8).ravel()
    buf = torch.full((device_bytes_before + raw.size + 256,), GUARD, dtype=torch.uint8, device=DEV)
    buf[device_bytes_before:device_bytes_before + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
    return buf[device_bytes_before:device_bytes_before + raw.size], buf


def guards_intact(buf, before, size):
    b = buf.cpu().numpy()
    return (b[:before] == GUARD).all() and (b[before + size:] == GUARD).all() and len(b) == before + size + 256


def canary_run(G, name, names, st, tm, mask, params):
    """The entry point with every output a view 4 bytes into a guard-filled buffer and state / to_move / mask views at odd byte
    offsets: the outputs, after checking every guard byte and that the inputs are as given."""
    nat = G._native
    f, stream = entry(G, DEV, name)
    n = len(st)
    ins = [guarded(off, a) for off, a in ((1, st), (3, tm), (5, mask))]
    assert all(v.data_ptr() % 2 == 1 for v, _ in ins)
    shapes = {k: (n, 54) if k in ("visits", "wins", "losses") else (n,) for k in names}
    outs = {k: guarded(4, np.full(shapes[k], -7, np.int32)) for k in names}
    assert all(v.data_ptr() % 8 == 4 for v, _ in outs.values())
    nat.check(f(*[v.data_ptr() for v, _ in ins], *params, *[outs[k][0].data_ptr() for k in names], n, stream), name)
    torch.cuda.synchronize()
    for (v, buf), off, a in zip(ins, (1, 3, 5), (st, tm, mask)):
        assert guards_intact(buf, off, a.size) and np.array_equal(v.cpu().numpy().view(np.int8).reshape(a.shape), a), name
    for k in names:
        assert guards_intact(outs[k][1], 4, 4 * int(np.prod(shapes[k]))), (name, k)
    return tuple(outs[k][0].cpu().numpy().view(np.int32).reshape(shapes[k]) for k in names)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_search_outputs_stay_inside_their_arrays(G, c5, n):
    st, tm = np.array(c5[0][:n]), np.array(c5[1][:n])
    mask = (np.random.default_rng(n).random((n, 54)) < 0.5).astype(np.int8)
    targs = (40, 6, 30, 64, 3, 17, 4)
    same(canary_run(G, "tree_search", NAMES, st, tm, mask, targs), device_run(G, st, tm, mask, *targs))
    pargs = (8, 30, 3, 17, 4)
    GP.same(canary_run(G, "playout_values", PLAYOUT_NAMES, st, tm, mask, pargs), GP.device_run(G, st, tm, mask, *pargs))


def test_each_search_output_null_in_turn(G, c5):
    n = 65
    st, tm = c5[0][:n], c5[1][:n]
    mask = (np.random.default_rng(n).random((n, 54)) < 0.5).astype(np.int8)
    for name, names, params, plain in (("tree_search", NAMES, (40, 6, 30, 64, 3, 17, 4), device_run),
                                       ("playout_values", PLAYOUT_NAMES, (8, 30, 3, 17, 4), GP.device_run)):
        full = dict(zip(names, plain(G, st, tm, mask, *params)))
        for missing in names:
            keep = [k for k in names if k != missing]
            got = search_some(G, DEV, name, names, st, tm, mask, params, keep)
            assert set(got) == set(keep)
            for k in keep:
                assert np.array_equal(got[k], full[k]), (name, missing, k)


def test_nonzero_bytes_are_set_bytes_on_the_device(G):
    """to_move and mask bytes of -128, -1, 2 and 127 are read as set: the 0 / 1 inputs' result, which is the restatement's."""
    st, tm, mask, tm2, mask2 = byte_value_boards()
    exp = restate(st, tm, mask, *TREE_BYTES)
    same(device_run(G, st, tm, mask, *TREE_BYTES), exp)
    same(device_run(G, st, tm2, mask2, *TREE_BYTES), exp)
    exp = PP.restate(st, tm, mask, *PLAYOUT_BYTES)
    GP.same(GP.device_run(G, st, tm, mask, *PLAYOUT_BYTES), exp)
    GP.same(GP.device_run(G, st, tm2, mask2, *PLAYOUT_BYTES), exp)
