"""gbl_tree_search / TreeSearchGobbletPolicy on the host flavour (no GPU): against a Python restatement of the contract
(include/gobblet_hip.h) built from the oracle's board functions and its masked-uniform sampler on generator stream 3, plus
properties, tactics, argument limits, the policy surface and an arena against the masked-random player."""
import math

import numpy as np
import pytest
import torch

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests.search_harness import TREE_NAMES as NAMES, run, same
from tests.test_playout_policy import (E40, UNCOVER_ACTION, UNCOVER_SEQ, WIN_ACTION, WIN_SEQ, arena, play, random_midgames,
                                       sample_stream)

STREAM_TREE = 3


def pid(g, i, j):
    return (g * 1024 + i) * 256 + j


def key(W, L, n, P, n_parent, explore):
    return (((W - L + n * P) << 15) // (n * P)) + ((explore * math.isqrt((n_parent.bit_length() << 20) // n)) >> 3)


class Node:
    def __init__(self, parent, action, term):
        self.parent, self.action, self.term = parent, action, term  # term: 0 open, 1 won / 2 lost by the side that moved in, 3 stuck
        self.children = {}  # action -> Node
        self.n = self.W = self.L = 0


def restate(state, to_move, mask, I, P, M, X, seed, env_base, call):
    """The contract, one iteration and one playout at a time, on the oracle."""
    n = len(state)
    visits, wins, losses = (np.zeros((n, 54), np.int32) for _ in range(3))
    action, nodes, plies = np.full(n, -1, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32)
    for b in range(n):
        g, mover = env_base + b, int(to_move[b] != 0)
        cand0 = oracle.legal_mask(state[b], mover) != 0
        if mask is not None:
            cand0 &= mask[b] != 0
        if not cand0.any():
            continue
        root = Node(None, -1, 0)
        for i in range(I):
            v, s, side, cand = root, state[b], mover, cand0
            while True:  # 1. select
                if v.term:
                    break
                untried = [int(a) for a in np.flatnonzero(cand) if int(a) not in v.children]
                if untried:
                    break
                best = max(sorted(v.children), key=lambda a: (key(v.children[a].W, v.children[a].L, v.children[a].n, P, v.n, X), -a))
                s, side, v = oracle.play_turn(s, side, best), 1 - side, v.children[best]
                cand = oracle.legal_mask(s, side) != 0
            if not v.term:  # 2. expand
                m = np.zeros(54, np.int8)
                m[untried] = 1
                a = sample_stream(m, seed, pid(g, i, 0), (call << 8) | 0, STREAM_TREE)
                s = oracle.play_turn(s, side, a)
                w = oracle.check_for_winner(s)
                mine = w if side == 0 else -w
                side = 1 - side
                term = 1 if mine > 0 else 2 if mine < 0 else (0 if oracle.legal_mask(s, side).any() else 3)
                v.children[a] = Node(v, a, term)
                v = v.children[a]
                nodes[b] += 1
            wl = [P if v.term == 1 else 0, P if v.term == 2 else 0]  # 3. evaluate
            for j in range(P if v.term == 0 else 0):
                q, sd, t, w = s, side, 0, 0
                while w == 0 and t < M:
                    t += 1
                    act = sample_stream(oracle.legal_mask(q, sd), seed, pid(g, i, j), (call << 8) | t, STREAM_TREE)
                    if act < 0:
                        break
                    q, sd = oracle.play_turn(q, sd, act), 1 - sd
                    plies[b] += 1
                    w = oracle.check_for_winner(q)
                mine = w if side == 1 else -w  # (for the side that moved INTO the leaf: 1 - side)
                wl[0] += mine > 0
                wl[1] += mine < 0
            while v.parent is not None:  # 4. back up
                v.n, v.W, v.L = v.n + 1, v.W + wl[0], v.L + wl[1]
                wl.reverse()
                v = v.parent
            root.n += 1
        for a, c in root.children.items():
            visits[b, a], wins[b, a], losses[b, a] = c.n, c.W, c.L
        action[b] = max(sorted(root.children), key=lambda a: (root.children[a].n, root.children[a].W - root.children[a].L, -a))
    return visits, wins, losses, action, nodes, plies


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def boards(golden_dir):  # (the 12 boards of tests/test_playout_policy.py)
    g = np.load(golden_dir + "/greedy.npz")
    st, tm = [np.zeros(27, np.int8)], [0]
    keep = np.flatnonzero(oracle.batch_winner(g["squares"]) == 0)[:4]
    st += list(g["squares"][keep])
    tm += list(g["to_move"][keep])
    ms, mt = random_midgames(7, seed=3)
    st += list(ms)
    tm += list(mt)
    st, tm = np.array(st, np.int8), np.array(tm, np.int8)
    assert len(st) == 12 and set(tm.tolist()) == {0, 1}
    return st, tm


@pytest.mark.parametrize("I,P,M,X,call,env_base", [
    (1, 1, 0, 0, 0, 0), (5, 3, 20, 128, 0, 0), (64, 4, 30, 128, 0, 0), (64, 4, 30, 0, 3, 7), (64, 4, 30, 1024, 0, E40),
    (200, 8, 255, 128, 5, E40)])
def test_host_flavour_equals_restatement(cpu, boards, I, P, M, X, call, env_base):
    st, tm = boards
    if I == 200:  # (the restatement walks every ply through ctypes: a third of the boards at the largest budget)
        st, tm = st[::3], tm[::3]
    same(run("tree_search", "cpu", st, tm, None, (I, P, M, X, 9, env_base, call)), restate(st, tm, None, I, P, M, X, 9, env_base, call))


def test_host_flavour_equals_restatement_with_mask(cpu, boards):
    st, tm = boards
    mask = (np.random.default_rng(2).random((len(st), 54)) < 0.4).astype(np.int8)
    mask[0] = 0  # a board without a candidate
    got = run("tree_search", "cpu", st, tm, mask, (48, 5, 40, 128, 1, 3, 2))
    same(got, restate(st, tm, mask, 48, 5, 40, 128, 1, 3, 2))
    assert got["action"][0] == -1 and got["nodes"][0] == 1 and got["plies"][0] == 0 and not got["visits"][0].any()


@pytest.fixture(scope="module")
def many():
    env = G.BatchedGobblet(300, "cpu", auto_reset=True, seed=11)
    env.rollout(37)
    st, tm = env.squares.numpy().copy(), env.to_move.numpy().copy()
    assert (oracle.batch_winner(st) == 0).all()
    return st, tm


def decide(v, w, l):
    """gbl_tree_search's decision rule from its outputs: most visits, then W - L, then the lowest action."""
    order = (v.astype(np.int64) << 32) + ((w.astype(np.int64) - l + (1 << 20)) << 6) + (63 - np.arange(54))
    return np.where((v > 0).any(1), np.argmax(np.where(v > 0, order, -1), 1), -1)


def test_properties(cpu, many):
    st, tm = many
    n, I, P = len(st), 48, 8
    legal = oracle.batch_legal_mask(st, tm) != 0
    mask = (np.random.default_rng(8).random((n, 54)) < 0.5).astype(np.int8)
    mask[5] = 0
    args = (P, 64, 128, 4)
    v, w, l, a, nd, p = run("tree_search", "cpu", st, tm, mask, (I, *args, 100, 1)).values()
    cand = legal & (mask != 0)
    has = cand.any(1)
    assert has.sum() > 290 and not has[5]
    assert (v.sum(1)[has] == I).all() and (v[~has] == 0).all()
    assert (w >= 0).all() and (l >= 0).all() and ((w + l) <= v * P).all()
    assert (v[~cand] == 0).all() and (w[~cand] == 0).all() and (l[~cand] == 0).all()
    assert (nd <= I + 1).all() and (nd[has] >= 2).all() and (nd[~has] == 1).all() and (p[~has] == 0).all()
    assert (a[~has] == -1).all() and np.array_equal(a, decide(v, w, l))
    assert (p <= I * P * 64).all()
    # no more iterations than candidates: every root child is visited at most once, and every iteration made a node
    few = int(cand.sum(1)[has].min())
    v1, _, _, _, nd1, _ = run("tree_search", "cpu", st, tm, mask, (few, *args, 100, 1)).values()
    assert np.isin(v1, (0, 1)).all() and (nd1[has] == few + 1).all()
    # a search is the beginning of every longer one
    v2, _, _, _, nd2, p2 = run("tree_search", "cpu", st, tm, mask, (2 * I, *args, 100, 1)).values()
    assert (nd2 >= nd).all() and (p2 >= p).all() and (v2.sum(1)[has] == 2 * I).all()
    assert (v2 >= v).all()  # (n_c of a root child only grows)
    # sharding over env_base changes nothing
    h = n // 3
    parts = [run("tree_search", "cpu", st[i:j], tm[i:j], mask[i:j], (I, *args, 100 + i, 1)) for i, j in ((0, h), (h, n))]
    for k, whole in zip(NAMES, (v, w, l, a, nd, p)):
        assert np.array_equal(np.concatenate([q[k] for q in parts]), whole), k
    # another call index searches otherwise; the same call twice gives the same
    v5 = run("tree_search", "cpu", st, tm, mask, (I, *args, 100, 5))["visits"]
    assert not np.array_equal(v5, v)
    same(run("tree_search", "cpu", st, tm, mask, (I, *args, 100, 1)), (v, w, l, a, nd, p))


def test_decided_root_moves(cpu):
    (sw, mw), (su, mu) = play(WIN_SEQ), play(UNCOVER_SEQ)
    I, P = 128, 8
    v, w, l, a, _, _ = run("tree_search", "cpu", np.array([sw, su]), np.array([mw, mu]), None, (I, P, 64, 128, 0, 0, 0)).values()
    assert a[0] == WIN_ACTION and v[0, WIN_ACTION] > 0 and w[0, WIN_ACTION] == v[0, WIN_ACTION] * P and l[0, WIN_ACTION] == 0
    assert a[1] != UNCOVER_ACTION and l[1, UNCOVER_ACTION] == v[1, UNCOVER_ACTION] * P and w[1, UNCOVER_ACTION] == 0


def winning_moves(s, side):
    """The legal actions of `side` after which check_for_winner() is `side`'s."""
    want = 1 if side == 0 else -1
    return [int(a) for a in np.flatnonzero(oracle.legal_mask(s, side)) if oracle.check_for_winner(oracle.play_turn(s, side, int(a))) == want]


def threat_positions(count, seed):
    """Midgame positions where the mover cannot win at once, the opponent WOULD win at once if it were to move, and only some
    root actions prevent that: (states, movers, per-position set of the preventing actions).  An action prevents it if it does not
    itself hand the opponent a line and leaves the opponent no winning reply."""
    out = []
    batch = 0
    while len(out) < count:
        st, tm = random_midgames(200, seed=seed + batch, min_plies=6, max_plies=16)
        batch += 1
        for s, m in zip(st, tm):
            m = int(m)
            if oracle.check_for_winner(s) != 0 or winning_moves(s, m) or not winning_moves(s, 1 - m):
                continue
            legal = [int(a) for a in np.flatnonzero(oracle.legal_mask(s, m))]
            safe = set()
            for a in legal:
                s2 = oracle.play_turn(s, m, a)
                if oracle.check_for_winner(s2) == 0 and not winning_moves(s2, 1 - m):
                    safe.add(a)
            if 0 < len(safe) < len(legal):
                out.append((s, m, safe))
            if len(out) == count:
                break
    return np.array([o[0] for o in out], np.int8), np.array([o[1] for o in out], np.int8), [o[2] for o in out]


# Measured on the host flavour on these 60 positions (default explore 16, max_plies 64, seed 0), actions chosen that do NOT parry:
# 6 at (256, 16), 0 at (512, 16) and (1024, 16); flat Monte-Carlo at the playouts of (512, 16), 256 per action, misses 16.  The
# record is profiles/r08/tree_policy.json "threat".
THREAT_BUDGET = (512, 16)


def test_depth2_threats_are_parried(cpu):
    st, tm, safe = threat_positions(60, seed=100)
    I, P = THREAT_BUDGET
    pol = G.TreeSearchGobbletPolicy(iterations=I, playouts=P, seed=0, device="cpu")
    a = pol.compute_actions_from_state(torch.from_numpy(st), torch.from_numpy(tm)).numpy()
    missed = [i for i in range(len(st)) if int(a[i]) not in safe[i]]
    assert not missed, missed


@pytest.mark.parametrize("flavour", ["cpu", "hip"])
def test_argument_limits(flavour):
    if flavour == "cpu":
        L = nat.cpu_raw()
        f, err = L.gbl_cpu_tree_search, L.gbl_cpu_last_error
    else:  # (the device entry point checks its arguments before any HIP call: no GPU needed)
        L = nat.lib()
        f, err = L.gbl_tree_search, L.gbl_last_error
    st, tm = np.zeros((2, 27), np.int8), np.zeros(2, np.int8)
    out = np.zeros(2, np.int32)

    def call(I=4, P=4, M=8, X=64, call=0, env_base=0, n=1):
        return f(st.ctypes.data, tm.ctypes.data, None, I, P, M, X, 0, env_base, call, None, None, None, out.ctypes.data, None, None, n, None)

    for kw, word in (({"I": 0}, b"iterations"), ({"I": 1025}, b"iterations"), ({"P": 0}, b"playouts"), ({"P": 257}, b"playouts"),
                     ({"M": -1}, b"max_plies"), ({"M": 256}, b"max_plies"), ({"X": -1}, b"explore"), ({"X": 1025}, b"explore"),
                     ({"call": 1 << 24}, b"call"), ({"env_base": (1 << 42) - 1, "n": 2}, b"2^42"), ({"env_base": 1 << 43}, b"2^42"),
                     ({"n": -1}, b"n < 0")):
        assert call(**kw) == nat.ERR_ARG, kw
        assert word in err(), (kw, err())
    assert f(None, tm.ctypes.data, None, 4, 4, 8, 64, 0, 0, 0, None, None, None, None, None, None, 1, None) == nat.ERR_ARG
    assert b"state" in err()
    assert call(n=0) == 0
    if flavour == "cpu":
        assert call(I=1024, P=256, M=255, X=1024, call=(1 << 24) - 1, env_base=(1 << 42) - 1, n=1) == 0 and out[0] >= 0
    for kw in ({"iterations": 0}, {"iterations": 1025}, {"playouts": 257}, {"max_plies": 256}, {"explore": 1025}):
        with pytest.raises(ValueError):
            G.TreeSearchGobbletPolicy(device="cpu", **kw)


def test_policy_surface_on_cpu(cpu, many):
    st, tm = many
    st, tm = torch.from_numpy(st[:40]), torch.from_numpy(tm[:40])
    obs = torch.from_numpy(np.stack([oracle.observe(s, int(m), int(m))["observation"] for s, m in zip(st.numpy(), tm.numpy())]))
    mask = torch.from_numpy(oracle.batch_legal_mask(st.numpy(), tm.numpy()))
    kw = dict(iterations=40, playouts=4, explore=96, seed=3, device="cpu")
    a = G.TreeSearchGobbletPolicy(**kw).compute_actions(obs, mask)
    b = G.TreeSearchGobbletPolicy(**kw).compute_actions_from_state(st, tm)
    assert a.dtype == torch.int32 and torch.equal(a, b)
    exp = run("tree_search", "cpu", st.numpy(), tm.numpy(), None, (40, 4, 64, 96, 3, 0, 0))
    assert np.array_equal(b.numpy(), exp["action"])
    pol = G.TreeSearchGobbletPolicy(**kw)
    val = pol.action_values(st, tm)
    last = (pol.last_visits, pol.last_wins, pol.last_losses, pol.last_action, pol.last_nodes, pol.last_plies)
    same(exp, [t.numpy() for t in last])
    seen = exp["visits"] > 0
    assert np.array_equal(val.numpy()[seen], ((exp["wins"] - exp["losses"])[seen] / (exp["visits"][seen] * 4.0)).astype(np.float32))
    assert np.isneginf(val.numpy()[~seen]).all()
    # the call index moves on once per call
    assert pol._calls == 1
    dist = pol.visit_distribution(st, tm)
    assert pol._calls == 2
    exp1 = run("tree_search", "cpu", st.numpy(), tm.numpy(), None, (40, 4, 64, 96, 3, 0, 1))
    assert dist.dtype == torch.float32 and np.array_equal(pol.last_visits.numpy(), exp1["visits"])
    assert np.allclose(dist.numpy(), exp1["visits"] / 40.0, rtol=1e-6, atol=0)  # (one float32 division: 2^-24 relative)
    assert np.allclose(dist.sum(1).numpy(), 1.0) and (dist.numpy()[mask.numpy() == 0] == 0).all()
    none = pol.visit_distribution(st[:2], tm[:2], torch.zeros((2, 54), dtype=torch.int8))  # boards without a candidate
    assert not none.any() and (pol.last_action == -1).all()
    # single-observation and rllib / tianshou shapes
    assert int(G.TreeSearchGobbletPolicy(**kw).compute_action(obs[0].numpy(), mask[0].numpy())) == int(b[0])
    r = G.TreeSearchGobbletPolicy(**kw).compute_actions_rllib({"observation": obs.numpy().reshape(40, -1), "action_mask": mask.numpy()})
    assert [int(x) for x in r] == b.tolist()
    f = G.TreeSearchGobbletPolicy(**kw).forward({"obs": {"obs": obs.numpy(), "mask": mask.numpy()}})
    assert f["act"].dtype == np.int64 and f["act"].tolist() == b.tolist()


# measured: the default constructor (256 iterations of 16 playouts, max_plies 64, seed 0) as player_1 wins ARENA_CPU_WINS of 256
# games against the masked-random player (seed 7)
ARENA_CPU_WINS = 255


def test_policy_on_cpu_beats_random(cpu):
    wins = arena(G.TreeSearchGobbletPolicy(seed=0, device="cpu"), 256, seed=7)
    assert wins >= 0.9 * 256  # (the floor, with a margin below the record)
    assert wins == ARENA_CPU_WINS
