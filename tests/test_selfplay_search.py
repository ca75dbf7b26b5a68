"""gbl_collect_search / gbl_outcome_targets on the host flavour (no GPU): whole games with the tree search on either or both sides
against a Python loop over plies -- the restatement of gbl_tree_search on the oracle (tests/test_tree_policy.py), a few-line
restatement of the visit-proportional draw, and the oracle's step with auto-reset -- plus properties, sharding, the outcome
targets against numpy, argument limits of both flavours and the Python surface on device="cpu"."""
import numpy as np
import pytest
import torch

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests.search_harness import replay_arg_errors, run
from tests.selfplay_harness import CODES, SCALARS, cells, host_collect, same, strides  # noqa: F401  (re-exported)
from tests.test_playout_policy import random_midgames, sample_stream
from tests.test_tree_policy import restate

STREAM_VISIT = 4
M32 = 0xFFFFFFFF


def word(seed, env_id, ply, stream):
    """The generator word of (seed, env_id, ply, stream): include/gobblet_hip.h, gbl_sample."""
    o = oracle.philox4x32_10([env_id & M32, env_id >> 32, ply >> 2, stream], [seed & M32, seed >> 32])
    return int(o[ply & 3])


def visits_draw(visits, r):
    """k = (r * S) >> 32; the lowest action whose running sum of visits exceeds k."""
    k = (r * int(visits.sum())) >> 32
    over = np.flatnonzero(np.cumsum(visits.astype(np.int64)) > k)
    return int(over[0]) if len(over) else -1


def collect(lib, st, tm, turn, T, pols, its, pls, M, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev=None, keep=None):
    """gbl_cpu_collect_search on host arrays through `lib`; returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    return host_collect("search", lib.gbl_cpu_collect_search, lib.gbl_cpu_last_error, st, tm, turn, T, pols, X, sample_plies, illegal_mode,
                        layout, seed, env_base, ply0, ply_dev, keep, its=its, pls=pls, M=M)


def restate_collect(st, tm, turn, T, pols, its, pls, M, X, sample_plies, illegal_mode, seed, env_base, ply0):
    """The contract of gbl_collect_search, ply by ply, on the oracle."""
    n = len(st)
    st, tm, dn = st.copy(), tm.copy(), np.zeros(n, np.int8)
    turn = np.zeros(n, np.int32) if turn is None else turn.astype(np.int32).copy()
    out = {k: [] for k, _, _ in SCALARS}
    for t in range(T):
        q = ply0 + t
        legal = oracle.batch_legal_mask(st, tm)
        actions, mover = np.zeros(n, np.int32), tm.copy()
        visits, value, nodes, how = np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int8)
        for b in range(n):
            m, g = int(tm[b]), env_base + b
            if pols[m] == "tree":
                v, w, l, a, nd, _ = restate(st[b:b + 1], tm[b:b + 1], None, its[m], pls[m], M, X, seed, g, q)
                visits[b], value[b], nodes[b] = v[0], int((w[0] - l[0]).sum()), nd[0]
                if turn[b] < sample_plies:
                    actions[b], how[b] = visits_draw(v[0], word(seed, g, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
                else:
                    actions[b], how[b] = a[0], nat.HOW_SEARCH
            else:
                actions[b] = sample_stream(legal[b], seed, g, q, 0)
        r = oracle.batch_step(st, tm, dn, actions, illegal_mode, auto_reset=True, turn=turn)
        for k, v in (("actions", actions), ("winner", r["winner"]), ("rewards", r["reward"]), ("done", dn.copy()), ("to_move", tm.copy()),
                     ("action_mask", r["mask"]), ("observation", r["obs"].reshape(n, 117)), ("visits", visits), ("value", value),
                     ("nodes", nodes), ("how", how), ("mover", mover)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, st, tm, dn, turn


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def boards():
    """12 midgame boards and two fresh ones, with the turn counters such games would have."""
    ms, mt = random_midgames(12, seed=5, min_plies=2, max_plies=14)
    assert (oracle.batch_winner(ms) == 0).all()
    st = np.concatenate([np.zeros((1, 27), np.int8), ms, np.zeros((1, 27), np.int8)])
    tm = np.concatenate([np.zeros(1, np.int8), mt, np.zeros(1, np.int8)]).astype(np.int8)
    turn = np.array([0] + [int((s != 0).sum()) for s in ms] + [0], np.int32)  # (at least the pieces on the board)
    assert len(st) == 14 and set(tm.tolist()) == {0, 1} and (turn < 4).sum() >= 3 and (turn >= 4).sum() >= 3
    return st, tm, turn


T = 12
GRID = [  # policies, iterations, playouts, sample_plies, illegal_mode, ply_dev
    (("tree", "tree"), (32, 32), (8, 8), 0, nat.ILLEGAL_NOOP, None),
    (("tree", "tree"), (48, 16), (4, 8), 4, nat.ILLEGAL_TERMINATE, 9),
    (("tree", "random"), (32, 32), (8, 8), 4, nat.ILLEGAL_NOOP, 3),
    (("random", "tree"), (32, 32), (8, 8), 0, nat.ILLEGAL_TERMINATE, None),
    (("tree", "random"), (48, 16), (4, 8), 0, nat.ILLEGAL_TERMINATE, None),
    (("random", "tree"), (48, 16), (4, 8), 4, nat.ILLEGAL_NOOP, 2),
]


@pytest.mark.parametrize("pols,its,pls,sample_plies,illegal_mode,ply_dev", GRID)
def test_host_flavour_equals_composition(cpu, boards, pols, its, pls, sample_plies, illegal_mode, ply_dev):
    st, tm, turn = boards
    M, X, seed, env_base, ply0 = 40, 128, 9, 7, 5
    exp = restate_collect(st, tm, turn, T, pols, its, pls, M, X, sample_plies, illegal_mode, seed, env_base, ply0 + (ply_dev or 0))
    for layout in ("time", "tile"):
        got = collect(cpu, st, tm, turn, T, pols, its, pls, M, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev)
        same(got, exp)
    assert exp[0]["done"].any() or pols != ("tree", "random")  # (the searching side finishes games against the random one)
    if sample_plies:
        assert (exp[0]["how"] == nat.HOW_SEARCH_SAMPLED).any() and (exp[0]["how"] == nat.HOW_SEARCH).any()


@pytest.fixture(scope="module")
def many():
    env = G.BatchedGobblet(200, "cpu", auto_reset=True, seed=11, track_turn=True)
    env.rollout(9)
    st, tm, turn = env.squares.numpy().copy(), env.to_move.numpy().copy(), env.turn.numpy().copy()
    assert (oracle.batch_winner(st) == 0).all()
    return st, tm, turn


def test_properties(cpu, many):
    st, tm, turn = many
    n, its, pls, sp = len(st), (24, 40), (4, 4), 3
    for pols in (("tree", "tree"), ("tree", "random"), ("random", "tree")):
        tr, s1, m1, d1, t1 = collect(cpu, st, tm, turn, 10, pols, its, pls, 40, 64, sp, nat.ILLEGAL_NOOP, "time", 3, 100, 0)
        mover, how, v, a = tr["mover"], tr["how"], tr["visits"].astype(np.int64), tr["actions"]
        tree = np.array([p == "tree" for p in pols])[mover]
        assert np.array_equal(how != nat.HOW_RANDOM, tree)
        assert (v.sum(2)[tree] == np.array(its)[mover][tree]).all() and (v[~tree] == 0).all()
        assert (tr["nodes"][~tree] == 0).all() and (tr["value"][~tree] == 0).all() and (tr["nodes"][tree] >= 2).all()
        # the decision is an action with the most visits; a sampled action was visited
        dec = how == nat.HOW_SEARCH
        picked = np.take_along_axis(v, a[..., None].astype(np.int64), 2)[..., 0]
        assert (picked[dec] == v.max(2)[dec]).all() and (picked[how == nat.HOW_SEARCH_SAMPLED] > 0).all()
        # ... the lowest such action when the search's own order (visits, then W - L, then the action) leaves only the action:
        # checked exactly against gbl_tree_search below
        # the mover of ply t is who was to move after ply t - 1, player_1 after a game's end
        assert np.array_equal(mover[0], tm) and np.array_equal(mover[1:], tr["to_move"][:-1])
        assert (tr["to_move"][tr["done"] != 0] == 0).all()
        # values are bounded by the games behind them
        games = v.sum(2) * np.array(pls)[mover]
        assert (np.abs(tr["value"]) <= games).all()
        assert np.array_equal(m1, tr["to_move"][-1]) and np.array_equal(d1, tr["done"][-1])
    # ply 0 of (tree, tree) IS gbl_tree_search(call = ply0) on the entry position, decision included
    from tests.test_tree_policy import run
    tr, *_ = collect(cpu, st, tm, turn, 1, ("tree", "tree"), (24, 24), (4, 4), 40, 64, 0, nat.ILLEGAL_NOOP, "time", 3, 100, 6)
    v, w, l, a, nd, _ = run("tree_search", "cpu", st, tm, None, (24, 4, 40, 64, 3, 100, 6)).values()
    assert np.array_equal(tr["visits"][0], v) and np.array_equal(tr["actions"][0], a) and np.array_equal(tr["nodes"][0], nd)
    assert np.array_equal(tr["value"][0], (w - l).sum(1))
    # arg-max of the visits under tree_final_key's order wherever the search decided
    key = (v.astype(np.int64) << 32) + ((w.astype(np.int64) - l + (1 << 18)) << 6) + (63 - np.arange(54))
    assert np.array_equal(tr["actions"][0], np.argmax(np.where(v > 0, key, -1), 1))


def test_sharding(cpu, many):
    st, tm, turn = many
    args = (8, ("tree", "random"), (20, 20), (4, 4), 30, 64, 2, nat.ILLEGAL_NOOP)
    for layout in ("time", "tile"):
        whole = collect(cpu, st, tm, turn, *args, layout, 3, 50, 2)
        a, k = 70, 90
        part = collect(cpu, st[a:a + k], tm[a:a + k], turn[a:a + k], *args, layout, 3, 50 + a, 2)
        for key in whole[0]:
            assert np.array_equal(part[0][key], whole[0][key][:, a:a + k]), key
        for g, e in zip(part[1:], whole[1:]):
            assert np.array_equal(g, e[a:a + k])


def test_tallies_and_null_outputs(cpu, many):
    st, tm, turn = many
    n, T_ = len(st), 6
    counters = np.zeros((nat.COUNTER_STRIPES, nat.COUNTER_STRIDE), np.int64)
    tr, *_ = host_collect("search", cpu.gbl_cpu_collect_search, cpu.gbl_cpu_last_error, st, tm, None, T_, ("tree", "random"), 64, 0,
                          nat.ILLEGAL_NOOP, "time", 1, 0, 0, keep=("winner", "done"), counters=counters, its=(16, 0), pls=(4, 0), M=30)
    tot = counters.sum(0)
    assert set(tr) == {"winner", "done"}
    assert tot[0] == n * T_ and tot[1] == tr["done"].sum() and tot[2] == (tr["winner"] == 1).sum() and tot[3] == (tr["winner"] == -1).sum()


# ---- gbl_outcome_targets ----------------------------------------------------------------------------------------------------
def targets_numpy(done, rewards, mover):
    """(T, n) arrays -> z, plies_left: the definition, one cell at a time."""
    Tn, n = done.shape
    z, left = np.full((Tn, n), nat.Z_OPEN, np.int8), np.full((Tn, n), -1, np.int16)
    for b in range(n):
        for t in range(Tn):
            ends = [e for e in range(t, Tn) if done[e, b]]
            if ends:
                z[t, b], left[t, b] = rewards[ends[0], b, mover[t, b]], ends[0] - t
    return z, left


def targets(lib, done, rewards, mover, layout, with_left=True):
    Tn, n = done.shape
    ps, ts, total = strides(n, Tn, layout)
    at = cells(n, Tn, layout)
    d, r, m = np.zeros(total, np.int8), np.zeros((total, 2), np.int8), np.zeros(total, np.int8)
    d[at], r[at], m[at] = done, rewards, mover
    z, left = np.full(total, 77, np.int8), np.full(total, 77, np.int16)
    rc = lib.gbl_cpu_outcome_targets(d.ctypes.data, r.ctypes.data, m.ctypes.data, z.ctypes.data, left.ctypes.data if with_left else None,
                                     n, ps, ts, Tn, None)
    assert rc == 0, lib.gbl_cpu_last_error()
    untouched = np.ones(total, bool)
    untouched[at] = False
    assert (z[untouched] == 77).all() and (left[untouched] == 77).all()  # (nothing outside the cells is written)
    return z[at], left[at]


@pytest.mark.parametrize("layout", ["time", "tile"])
def test_outcome_targets(cpu, many, layout):
    st, tm, turn = many
    # a recorded trajectory with game ends (tree against random), in both illegal modes' reward conventions
    tr, *_ = collect(cpu, st, tm, turn, 24, ("tree", "random"), (16, 16), (4, 4), 30, 64, 0, nat.ILLEGAL_NOOP, "time", 3, 0, 0)
    assert tr["done"].sum() > 20
    z, left = targets(cpu, tr["done"], tr["rewards"], tr["mover"], layout)
    ez, el = targets_numpy(tr["done"], tr["rewards"], tr["mover"])
    assert np.array_equal(z, ez) and np.array_equal(left, el)
    assert set(np.unique(z).tolist()) <= {-1, 1, nat.Z_OPEN} and (z == 1).any() and (z == -1).any() and (z == nat.Z_OPEN).any()
    assert np.array_equal(targets(cpu, tr["done"], tr["rewards"], tr["mover"], layout, with_left=False)[0], ez)
    # hand-made: an end on the first ply, on the last ply, none, two in the window, an illegal-terminate end (mover -1, other 0)
    Tn, n = 6, 70
    done, rewards = np.zeros((Tn, n), np.int8), np.zeros((Tn, n, 2), np.int8)
    mover = (np.arange(Tn)[:, None] + np.arange(n)) % 2
    done[0, 0], rewards[0, 0] = 1, (1, -1)
    done[Tn - 1, 1], rewards[Tn - 1, 1] = 1, (-1, 1)
    done[1, 3], rewards[1, 3] = 1, (-1, 1)
    done[4, 3], rewards[4, 3] = 1, (1, -1)
    done[2, 65], rewards[2, 65] = 1, (0, -1)
    rewards[3, 2] = (1, -1)  # a reward without a game end is not an outcome
    z, left = targets(cpu, done, rewards, mover.astype(np.int8), layout)
    ez, el = targets_numpy(done, rewards, mover)
    assert np.array_equal(z, ez) and np.array_equal(left, el)
    assert (z[:, 2] == nat.Z_OPEN).all() and (left[:, 2] == -1).all() and (z[1:, 0] == nat.Z_OPEN).all() and left[0, 0] == 0
    assert (left[:, 1] == np.arange(Tn)[::-1]).all() and list(left[:, 3]) == [1, 0, 2, 1, 0, -1]
    assert set(z[:3, 65].tolist()) == {0, -1} and z[0, 3] == rewards[1, 3, mover[0, 3]]


# ---- argument limits ----------------------------------------------------------------------------------------------------------
def test_argument_precedence_replays_the_recorded_table(golden_dir):
    """tests/golden/selfplay_arg_errors.json (scripts/record_selfplay_arg_errors.py): for each of the four self-play entry points
    and both flavours every check alone, every adjacent pair of checks broken together (the earlier one answers), a clean call and
    the n == 0 / plies == 0 returns in front of arguments a later check refuses -- code and message as recorded."""
    import json
    import os
    table = json.load(open(os.path.join(golden_dir, "selfplay_arg_errors.json")))
    per_fn = {fn: sum(c["fn"] == fn for c in table) for fn in ("collect_search", "collect_search_eval", "collect_search_solve", "collect_search_noise")}
    assert sum(per_fn.values()) == len(table) and min(per_fn.values()) >= 50, per_fn
    assert sum(c["host"] is None for c in table) >= 40 and sum(c["device"][0] == 0 for c in table) >= 12
    replay_arg_errors(table)


@pytest.mark.parametrize("flavour", ["cpu", "hip"])
def test_argument_limits(flavour):
    if flavour == "cpu":
        L = nat.cpu_raw()
        f, tg, cp, err = L.gbl_cpu_collect_search, L.gbl_cpu_outcome_targets, L.gbl_cpu_collect_policy, L.gbl_cpu_last_error
    else:  # (the device entry points check their arguments before any HIP call: no GPU needed)
        L = nat.lib()
        f, tg, cp, err = L.gbl_collect_search, L.gbl_outcome_targets, L.gbl_collect_policy, L.gbl_last_error
    n, T_ = 2, 2
    st, tm, dn = np.zeros((64, 27), np.int8), np.zeros(64, np.int8), np.zeros(64, np.int8)
    turn = np.zeros(64, np.int32)
    buf = np.zeros(64 * 1024, np.int8)  # (16-byte aligned below; large enough for two plies of every array)
    base = (buf.ctypes.data + 15) & ~15

    def call(p0=nat.POLICY_TREE, p1=nat.POLICY_TREE, I0=4, I1=4, P0=2, P1=2, M=8, X=64, sp=0, mode=0, ply0=0, plies=T_, env_base=0, n=n,
             ps=64, ts=64, turn=None, state=st.ctypes.data, actions=None, mask=None, visits=None, reward=None):
        return f(state, tm.ctypes.data, dn.ctypes.data, actions, None, reward, None, None, mask, None, visits, None, None, None, None, n, ps, ts,
                 0, env_base, ply0, None, plies, p0, p1, I0, I1, P0, P1, M, X, sp, mode, None, turn, None)

    for kw, w in (({"I0": 0}, b"iterations"), ({"I1": 1025}, b"iterations"), ({"P0": 0}, b"playouts"), ({"P1": 257}, b"playouts"),
                  ({"M": -1}, b"max_plies"), ({"M": 256}, b"max_plies"), ({"X": -1}, b"explore"), ({"X": 1025}, b"explore"),
                  ({"sp": -1}, b"sample_plies"), ({"sp": 2}, b"turn"), ({"mode": 2}, b"illegal_mode"),
                  ({"ply0": (1 << 24) - 1}, b"2^24"), ({"ply0": 1 << 24, "plies": 1}, b"2^24"),
                  ({"env_base": (1 << 42) - 1}, b"2^42"), ({"n": -1}, b"n < 0"), ({"state": None}, b"state"),
                  ({"p0": nat.POLICY_GREEDY1}, b"policy"), ({"p1": nat.POLICY_GREEDY2}, b"policy"), ({"p0": nat.POLICY_GREEDY3}, b"policy"),
                  ({"p1": 5}, b"policy"), ({"p0": -1}, b"policy"),
                  ({"ps": 8}, b"stride"), ({"ps": 64, "ts": 64, "n": 65}, b"stride"), ({"ps": 72}, b"stride"), ({"ts": 0}, b"stride")):
        assert call(**kw) == nat.ERR_ARG, kw
        assert w in err(), (kw, err())
    # a random side's pair is not read
    assert call(p1=nat.POLICY_RANDOM, I1=0, P1=0, n=0) == 0 and call(n=0) == 0 and call(plies=0) == 0
    if flavour == "hip":  # (alignment is the device flavour's business: its row stores are 16-byte vectors)
        for kw, w in (({"mask": base + 8}, b"mask_traj"), ({"actions": base + 2}, b"4-byte"), ({"visits": base + 1}, b"visits_traj"),
                      ({"reward": base + 1}, b"reward_traj"), ({"state": base + 4}, b"state")):
            assert call(**kw) == nat.ERR_ALIGN, kw
            assert w in err(), (kw, err())
    else:
        assert call(turn=turn.ctypes.data, sp=2, I0=1024, P0=2, I1=3, P1=256, M=255, X=1024, ply0=(1 << 24) - T_, env_base=(1 << 42) - n,
                    actions=base) == 0
    # gbl_collect_policy keeps rejecting the tree's code
    hist = np.full((64, 2, 3), -1, np.int8)
    for p0, p1 in ((nat.POLICY_TREE, 0), (0, nat.POLICY_TREE)):
        assert cp(st.ctypes.data, tm.ctypes.data, dn.ctypes.data, hist.ctypes.data, *[None] * 10, n, 64, 64, 0, 0, 0, None, 1, p0, p1, 0, 0,
                  None, None, None) == nat.ERR_ARG
        assert b"policy" in err()
    # gbl_outcome_targets
    d = base

    def tcall(done=d, reward=d + 4096, mover=d + 8192, z=d + 12288, left=d + 16384, n=n, ps=64, ts=64, plies=T_):
        return tg(done, reward, mover, z, left, n, ps, ts, plies, None)

    for kw, w in (({"done": None}, b"done_traj"), ({"reward": None}, b"reward_traj"), ({"mover": None}, b"mover_traj"), ({"z": None}, b"z_traj"),
                  ({"n": -1}, b"n < 0"), ({"ps": 8}, b"stride"), ({"plies": 32768}, b"32767")):
        assert tcall(**kw) == nat.ERR_ARG, kw
        assert w in err(), (kw, err())
    assert tcall(n=0) == 0 and tcall(plies=0) == 0
    if flavour == "hip":
        assert tcall(reward=d + 4097) == nat.ERR_ALIGN and tcall(left=d + 16385) == nat.ERR_ALIGN
    else:
        assert tcall(left=None) == 0


# ---- the Python surface on device="cpu" -------------------------------------------------------------------------------------------
def test_python_surface_on_cpu(cpu):
    kw = dict(iterations=(24, 16), playouts=4, max_plies=30, explore=64, sample_plies=2)
    env = G.BatchedGobblet(70, "cpu", auto_reset=True, seed=4, env_base=3, track_turn=True)
    env.rollout(5)
    st, tm, turn, ply = env.squares.numpy().copy(), env.to_move.numpy().copy(), env.turn.numpy().copy(), env.ply
    for layout in ("time", "tile"):
        e = G.BatchedGobblet(70, "cpu", auto_reset=True, seed=4, env_base=3, track_turn=True)
        e.load_state_dict(env.state_dict())
        out = e.collect(6, policies=("tree", "tree"), search=kw, layout=layout, count=True)
        assert {"visits", "value", "nodes", "how", "mover"} <= set(out) and e.ply == ply + 6
        exp = collect(cpu, st, tm, turn, 6, ("tree", "tree"), (24, 16), (4, 4), 30, 64, 2, nat.ILLEGAL_NOOP, layout, 4, 3, ply)

        def view(k):
            v = out[k].numpy()
            if layout == "tile":  # (tiles, plies, 64, ...) -> (plies, n, ...)
                v = np.moveaxis(v, 1, 0).reshape((6, -1) + v.shape[3:])[:, :70]
            return v.reshape(exp[0][k].shape)
        for k in exp[0]:
            assert np.array_equal(view(k), exp[0][k]), k
        assert np.array_equal(e.squares.numpy(), exp[1]) and np.array_equal(e.turn.numpy(), exp[4])
        assert np.array_equal(e.action_mask.numpy(), exp[0]["action_mask"][-1]) and int(e.counters[0]) == 70 * 6
        e.outcome_targets(out)
        ez, el = targets_numpy(exp[0]["done"], exp[0]["rewards"], exp[0]["mover"])
        assert out["z"].dtype == torch.int8 and out["plies_left"].dtype == torch.int16
        if layout == "time":
            assert np.array_equal(out["z"].numpy(), ez) and np.array_equal(out["plies_left"].numpy(), el)
    # a policy instance supplies its parameters; "tree" against "random"; buffers of the caller's own
    pol = G.TreeSearchGobbletPolicy(iterations=12, playouts=3, max_plies=20, explore=32, device="cpu")
    e = G.BatchedGobblet(70, "cpu", auto_reset=True, seed=4, env_base=3, track_turn=True)
    e.load_state_dict(env.state_dict())
    buf = e.trajectory_buffers(4, search_outputs=True)
    out = e.collect(4, out=buf, policies=("random", pol))
    exp = collect(cpu, st, tm, turn, 4, ("random", "tree"), (1, 12), (1, 3), 20, 32, 0, nat.ILLEGAL_NOOP, "time", 4, 3, ply)
    for k in exp[0]:
        assert np.array_equal(out[k].numpy().reshape(exp[0][k].shape), exp[0][k]), k
    assert "tree" in G.BatchedGobblet.POLICIES
    for bad in (dict(policies=("tree", "greedy"), search=kw), dict(policies=("greedy", "random"), search=kw),
                dict(policies=("tree", "tree"), search=dict(depth=3)), dict(policies=("tree", "tree"), search=dict(iterations=2000)),
                dict(policies=("tree", "tree"), opening_plies=2)):
        with pytest.raises(ValueError):
            e.collect(2, **bad)
    with pytest.raises(ValueError):
        G.BatchedGobblet(8, "cpu", auto_reset=True).collect(2, policies=("tree", "tree"), search=dict(sample_plies=1))
    with pytest.raises(ValueError):
        e.outcome_targets(e.collect(2))


def test_greedy_pairs_still_go_to_collect_policy(cpu):
    """policies without "tree" behave as before: exactly a direct gbl_cpu_collect_policy call."""
    n, T_ = 70, 5
    env = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=6, track_turn=True)
    env.rollout(4)
    sd = env.state_dict()
    out = env.collect(T_, policies=("greedy", "random"), opening_plies=2)
    assert {"chosen", "how"} <= set(out) and "visits" not in out
    st, tm, dn, tn = sd["squares"].numpy().copy(), sd["to_move"].numpy().copy(), sd["done"].numpy().copy(), sd["turn"].numpy().copy()
    hist = np.full((n, 2, 3), -1, np.int8)
    slot = out["_ply_stride"]
    arr = {k: np.zeros((T_, slot) + tail, dt) for k, dt, tail in SCALARS[:7]}
    chosen, how = np.zeros((T_, slot), np.int32), np.zeros((T_, slot), np.int8)
    rc = cpu.gbl_cpu_collect_policy(st.ctypes.data, tm.ctypes.data, dn.ctypes.data, hist.ctypes.data, *[arr[k].ctypes.data for k, _, _ in SCALARS[:7]],
                                    chosen.ctypes.data, how.ctypes.data, None, n, slot, 64, 6, 0, sd["ply"], None, T_, nat.POLICY_GREEDY2,
                                    nat.POLICY_RANDOM, 2, nat.ILLEGAL_NOOP, None, tn.ctypes.data, None)
    assert rc == 0
    for k, _, _ in SCALARS[:7]:
        assert np.array_equal(out[k].numpy().reshape(T_, n, -1), arr[k][:, :n].reshape(T_, n, -1)), k
    assert np.array_equal(out["chosen"].numpy(), chosen[:, :n]) and np.array_equal(out["how"].numpy(), how[:, :n])
    assert np.array_equal(env.squares.numpy(), st) and np.array_equal(env.policy_hist.numpy(), hist)


def test_example_runs_on_the_host_flavour():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "examples/example_selfplay_search.py", "cpu"], cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "one (obs, pi, z) tuple" in r.stdout and "games finished" in r.stdout
