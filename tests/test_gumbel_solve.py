"""gbl_collect_gumbel_solve on the host flavour (no GPU): Gumbel self-play with the exact solver in front of every search.  Against
the ply-by-ply loop on the host flavour's own entry points (gbl_cpu_solve -> the proven pick, or gbl_cpu_tree_search_gumbel(mask = C,
call = q) / gbl_cpu_tree_search_eval(mask = C) -> gbl_cpu_step_into) with every branch counted; against a Python restatement of the
rule; the two identities (depths 0: gbl_cpu_collect_search_gumbel, considered 0: gbl_cpu_collect_search_solve), a split window, two
shards and *ply_dev; the guard's property read off the trajectory alone; the consumers; the argument errors of both flavours in the
prologue's order; the declaration in both headers against the table in _native.py; and collect()'s spelling.

Positions: the fixture of every search test, BatchedGobblet(..., seed=11, track_turn=True).rollout(64).  Networks: smoke()'s seeded
integer evaluator (H = 64) and a second one of 128 hidden units."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests import solver_restatement as SR
from tests.gumbel_harness import host_collect_gumbel
from tests.gumbel_solve_harness import (BRANCHES, CASES, CENSUS, ENTRY, EXPLORE, SMALLEST_C, call_args, census, composed_loop, host_collect_gs,
                                        restate_collect_gs)
from tests.search_harness import run
from tests.selfplay_harness import SOLVE_NAMES, _evaluator, host_collect, same
from tests.test_gumbel_search import Counting
from tests.test_selfplay_solve import fixture_boards, six_boards, smoke_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, ENV_BASE, PLY0, T = 0xFEDCBA9876543210, (1 << 41) + 77, 3, 6


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def c5():
    return fixture_boards(65)


@pytest.fixture(scope="module")
def nets():
    return {64: smoke_net(), 128: R.random_net(128, 77)}


def test_the_fixtures_first_ply_is_the_issues_table(cpu):
    """gbl_cpu_solve alone: the five numbers per (boards, depth), and the smallest |C|."""
    st, tm, _ = fixture_boards(130)
    for (n, depth), row in CENSUS.items():
        got, smallest = census(st[:n], tm[:n], depth)
        assert tuple(int(x) for x in got) == row, (n, depth, got)
        if depth == 3:
            assert smallest == SMALLEST_C[n]


# (case, layout, sample_plies, gumbel_noise, scale, hidden, illegal_mode): every case in both layouts; the PUCT side of case 1 with and
# without sampled plies; noise 0 / 1, scale 0 / 23, H = 64 / 128 and both illegal modes spread over them
LOOPS = [(0, "time", 0, 1, 23, 64, nat.ILLEGAL_NOOP), (0, "tile", 0, 0, 0, 128, nat.ILLEGAL_TERMINATE),
         (1, "time", 0, 1, 23, 128, nat.ILLEGAL_TERMINATE), (1, "tile", 2, 0, 23, 64, nat.ILLEGAL_NOOP),
         (1, "time", 2, 1, 0, 64, nat.ILLEGAL_NOOP), (1, "tile", 0, 1, 23, 64, nat.ILLEGAL_NOOP),
         (2, "time", 0, 1, 0, 128, nat.ILLEGAL_NOOP), (2, "tile", 0, 0, 23, 64, nat.ILLEGAL_TERMINATE),
         (3, "time", 0, 1, 23, 64, nat.ILLEGAL_TERMINATE), (3, "tile", 0, 1, 0, 128, nat.ILLEGAL_NOOP)]
# the branches a case must meet on 65 boards x 6 plies (BRANCHES' names)
MEETS = {0: BRANCHES[:5], 1: BRANCHES[:6], 2: BRANCHES[:5] + ("unguarded rule",), 3: BRANCHES[:5] + ("random",)}


@pytest.mark.parametrize("case,layout,sample_plies,noise,scale,hidden,illegal_mode", LOOPS)
def test_host_flavour_equals_the_ply_by_ply_loop(cpu, c5, nets, case, layout, sample_plies, noise, scale, hidden, illegal_mode):
    pols, considered, deps, its = CASES[case]
    st, tm, turn = c5[0], c5[1], c5[2] % 5
    net = nets[hidden]
    use = tuple(net if p == "eval" else None for p in pols)
    got = host_collect_gs(st, tm, turn, T, pols, use, its, deps, considered, noise, 50, scale, EXPLORE, sample_plies, illegal_mode, layout, SEED,
                          ENV_BASE, PLY0)
    *exp, met = composed_loop(cpu, st, tm, turn, T, pols, (net, net), its, deps, considered, noise, 50, scale, EXPLORE, sample_plies,
                              illegal_mode, SEED, ENV_BASE, PLY0)
    assert set(got[0]) == {k for k, _, _ in SOLVE_NAMES} and len(got[0]) == 16
    same(got, exp)
    print("case %d: %s" % (case, met))
    assert all(met[k] > 0 for k in MEETS[case]), met
    how = got[0]["how"]
    assert set(np.unique(how).tolist()) <= {nat.HOW_RANDOM, nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED, nat.HOW_PROVEN, nat.HOW_GUMBEL}
    if case == 1:
        assert ((how == nat.HOW_SEARCH_SAMPLED).any()) == bool(sample_plies)


@pytest.mark.parametrize("illegal_mode", [nat.ILLEGAL_NOOP, nat.ILLEGAL_TERMINATE])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_flavour_equals_restatement(cpu, c5, nets, case, illegal_mode):
    pols, considered, deps, its = CASES[case]
    its = tuple(min(x, 8) for x in its)  # (the restatement walks its trees in Python)
    st, tm, turn = six_boards(c5)
    net = nets[64]
    use = tuple(net if p == "eval" else None for p in pols)
    exp = restate_collect_gs(st, tm, turn, 4, pols, (net, net), its, deps, considered, 1, 50, 23, EXPLORE, 2, illegal_mode, 9, (1 << 40) - 20, 8)
    for layout, ply_dev in (("time", None), ("tile", 3)):
        got = host_collect_gs(st, tm, turn, 4, pols, use, its, deps, considered, 1, 50, 23, EXPLORE, 2, illegal_mode, layout, 9, (1 << 40) - 20,
                              8 - (ply_dev or 0), ply_dev=ply_dev)
        same(got, exp)


def test_identities(cpu, c5, nets):
    st, tm, turn = c5[0], c5[1], c5[2] % 5
    L = cpu
    pair = (nets[64], nets[128])
    for layout in ("time", "tile"):
        # both depths 0: every shared array is gbl_cpu_collect_search_gumbel's; the guard's two are empty
        got = host_collect_gs(st, tm, turn, T, ("eval", "eval"), pair, (8, 16), (0, 0), (16, 0), 1, 50, 23, EXPLORE, 3, nat.ILLEGAL_NOOP, layout,
                              SEED, ENV_BASE, PLY0)
        assert (got[0].pop("outcomes") == SR.NONE).all() and (got[0].pop("proven") == 0).all()
        same(got, host_collect_gumbel(st, tm, turn, T, ("eval", "eval"), pair, (8, 16), (16, 0), 1, 50, 23, EXPLORE, 3, nat.ILLEGAL_NOOP, layout,
                                      SEED, ENV_BASE, PLY0))
        # both considered 0: every array is gbl_cpu_collect_search_solve's, whatever the rule's three say
        got = host_collect_gs(st, tm, turn, T, ("eval", "eval"), pair, (8, 16), (2, 3), (0, 0), 5, -3, 999, EXPLORE, 3, nat.ILLEGAL_TERMINATE,
                              layout, SEED, ENV_BASE, PLY0)
        same(got, host_collect("solve", L.gbl_cpu_collect_search_solve, L.gbl_cpu_last_error, st, tm, turn, T, ("eval", "eval"), EXPLORE, 3,
                               nat.ILLEGAL_TERMINATE, layout, SEED, ENV_BASE, PLY0, nets=pair, its=(8, 16), deps=(2, 3)))
    # a RANDOM side's depth and considered are not read
    got = host_collect_gs(st, tm, turn, T, ("random", "eval"), (None, pair[1]), (0, 8), (77, 0), (99, 4), seed=SEED, ply0=PLY0)
    assert (got[0].pop("outcomes") == SR.NONE).all() and (got[0].pop("proven") == 0).all()
    same(got, host_collect_gumbel(st, tm, turn, T, ("random", "eval"), (None, pair[1]), (0, 8), (0, 4), X=EXPLORE, seed=SEED, ply0=PLY0))


def test_split_window_shards_and_ply_dev(cpu, nets):
    st, tm, turn = fixture_boards(130)
    turn = turn % 5
    pair = (nets[64], nets[128])
    args = (("eval", "eval"), pair, (8, 16), (2, 3), (16, 4))
    kw = dict(sample_plies=3, seed=SEED)
    whole = host_collect_gs(st, tm, turn, T, *args, ply0=PLY0, **kw)
    # two shards through env_base
    halves = [host_collect_gs(st[a:b], tm[a:b], turn[a:b], T, *args, env_base=a, ply0=PLY0, **kw) for a, b in ((0, 65), (65, 130))]
    for k, v in whole[0].items():
        assert np.array_equal(v, np.concatenate([h[0][k] for h in halves], axis=1)), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(whole[i], np.concatenate([h[i] for h in halves]))
    # the window in two calls through ply0: the second goes on from the first's boards and turn counters
    first = host_collect_gs(st, tm, turn, 2, *args, ply0=PLY0, **kw)
    second = host_collect_gs(first[1], first[2], first[4], T - 2, *args, ply0=PLY0 + 2, **kw)
    for k, v in whole[0].items():
        assert np.array_equal(v, np.concatenate([first[0][k], second[0][k]])), k
    for i in (1, 2, 4):
        assert np.array_equal(whole[i], second[i])
    # *ply_dev
    same(host_collect_gs(st, tm, turn, T, *args, ply0=0, ply_dev=PLY0, **kw), whole)
    other = host_collect_gs(st, tm, turn, T, *args, ply0=PLY0 + 1, **kw)
    assert not np.array_equal(other[0]["visits"], whole[0]["visits"])  # (the Gumbel row moves with the ply index)
    # counters: the plies and the finished games of the window
    counters = np.zeros(nat.COUNTER_STRIPES * nat.COUNTER_STRIDE, np.int64)
    got = host_collect_gs(st, tm, turn, T, *args, ply0=PLY0, counters=counters, **kw)
    same(got, whole)
    tally = counters.reshape(nat.COUNTER_STRIPES, nat.COUNTER_STRIDE).sum(0)
    assert tally[0] == 130 * T and tally[1] == whole[0]["done"].sum()


def guard_property(tr, pols, deps, considered):
    """Off the trajectory alone, for every ply of a guarded side: a proven win at hand => the played action carries the best such
    verdict by the solver's key (the shortest win; the lowest action on ties) and how is 5; nothing proven => the played action's
    outcome is 0, the visits bytes are 1 .. 255 exactly on the outcome-0 actions and how is 10 (a side that follows the rule)."""
    out, V, how, act, vis, mover = (tr[k].astype(np.int64) for k in ("outcomes", "proven", "how", "actions", "visits", "mover"))
    counts = dict(wins=0, losses=0, unproven=0)
    for side in (0, 1):
        if pols[side] != "eval" or not deps[side]:
            assert (out[mover == side] == SR.NONE).all() and (V[mover == side] == 0).all()
            continue
        o, v, h, a, row = (x[mover == side] for x in (out, V, how, act, vis))
        assert (o != SR.NONE).any(1).all()
        played = o[np.arange(len(a)), a]
        has_win = (o > 0).any(1)
        best = np.where(o > 0, o, 1000).min(1)
        assert (played[has_win] == best[has_win]).all() and (h[has_win] == nat.HOW_PROVEN).all()
        assert (a[has_win] == np.where(o > 0, o, 1000).argmin(1)[has_win]).all()  # (the lowest action among the shortest wins)
        assert ((v > 0) == has_win).all()
        lost = ~has_win & ~(o == 0).any(1)
        assert ((v < 0) == lost).all() and (h[lost] == nat.HOW_PROVEN).all()
        assert (played[lost] == np.where(o == SR.NONE, 1000, o).min(1)[lost]).all()  # (every candidate loses: the longest loss)
        open_ = ~has_win & ~lost
        assert (v[open_] == 0).all() and (played[open_] == 0).all()
        if considered[side]:
            assert (h[open_] == nat.HOW_GUMBEL).all()
            on = o[open_] == 0
            assert ((row[open_] >= 1) & (row[open_] <= 255))[on].all() and (row[open_][~on] == 0).all()
        else:
            assert np.isin(h[open_], (nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED)).all()
        counts["wins"] += int(has_win.sum())
        counts["losses"] += int(lost.sum())
        counts["unproven"] += int(open_.sum())
    return counts


def test_guard_property(cpu, c5, nets):
    st, tm, turn = c5[0], c5[1], c5[2] % 6
    for case in range(len(CASES)):
        pols, considered, deps, its = CASES[case]
        use = tuple(nets[64] if p == "eval" else None for p in pols)
        tr = host_collect_gs(st, tm, turn, 8, pols, use, its, deps, considered, sample_plies=3, seed=5)[0]
        counts = guard_property(tr, pols, deps, considered)
        assert counts["wins"] >= 5 and counts["losses"] >= 1 and counts["unproven"] >= 5, counts  # (the property was put to the test)


def test_the_consumers_keep_the_proven_and_the_gumbel_plies(cpu, nets):
    n, plies, its = 130, 8, 16
    ev = _evaluator(nets[64])
    env = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=11, track_turn=True)
    env.rollout(40)
    tr = env.collect(plies, policies=("evaluator", "random"), out="fresh",
                     search=dict(evaluator=ev, iterations=its, explore=EXPLORE, gumbel=dict(considered=16, solve_depth=3)))
    env.outcome_targets(tr)
    how, z, done = tr["how"].numpy(), tr["z"].numpy(), tr["done"].numpy()
    assert set(np.unique(how).tolist()) == {nat.HOW_RANDOM, nat.HOW_PROVEN, nat.HOW_GUMBEL}
    valid = np.zeros_like(how, bool)
    valid[1:] = (z[1:] != nat.Z_OPEN) & (done[:-1] == 0)
    keep = valid & np.isin(how, (nat.HOW_PROVEN, nat.HOW_GUMBEL))  # the kept rows: exactly the valid cells with how 5 or 10
    K = int(keep.sum())
    assert (keep & (how == nat.HOW_PROVEN)).sum() > 20 and (keep & (how == nat.HOW_GUMBEL)).sum() > 20 and (valid & (how == 0)).sum() > 20
    rows = tr["visits"].numpy()
    assert (rows[how == nat.HOW_PROVEN].sum(1) == its).all() and (rows[how == nat.HOW_GUMBEL].sum(1) >= 255).all()
    assert not rows[how == nat.HOW_RANDOM].any()
    buf = G.ReplayBuffer(2048, "cpu")
    buf.append(env, tr, tag=3)
    assert buf.total == K
    at = np.argwhere(keep)
    tt, bb = at[:, 0], at[:, 1]
    assert np.array_equal(buf.visits[:K].numpy(), rows[tt, bb]) and np.array_equal(buf.z[:K].numpy(), z[tt, bb])
    drawn = buf.batch(256, symmetries=None, call=1, seed=5)
    slot = drawn["index"][:, 0].numpy()
    assert (slot >= 0).all() and np.array_equal(drawn["visits"].numpy(), rows[tt[slot], bb[slot]])
    stats = G.GobbletTrainer(64, "cpu", seed=1).step(drawn)
    assert int(stats[2]) == 256 and np.isfinite(stats.numpy()).all() and float(stats[0]) > 0.0
    tb = env.training_batch(tr, 256, symmetries=None, call=2)
    t_, b_ = tb["index"][:, 0].numpy(), tb["index"][:, 1].numpy()
    ok = t_ >= 0
    assert ok.sum() > 64 and keep[t_[ok], b_[ok]].all()
    seen = how[t_[ok], b_[ok]]
    assert (seen == nat.HOW_PROVEN).any() and (seen == nat.HOW_GUMBEL).any()


CONSIDERED_MSG = b"considered0 / considered1 must be in [0, 54]"
DEPTH_MSG = b"solve_depth0 / solve_depth1 must be in [0, 6]"
ERRORS = [  # (name, overrides, message or None: GBL_OK), in the prologue's order: collect_solve_error, considered, the rule's three, the pointers
    ("n < 0 before all", dict(n=-1, deps=(7, 0), considered=(55, 0)), b"n < 0"),
    ("iterations before the depth", dict(its=(0, 5), deps=(7, 0)), b"iterations must be in [1, 512]"),
    ("a depth of 7", dict(deps=(7, 2), considered=(55, 4), noise=2), DEPTH_MSG),
    ("a depth of 7, the other side", dict(deps=(0, 7), scale=65), DEPTH_MSG),
    ("a depth of -1", dict(deps=(-1, 2)), DEPTH_MSG),
    ("considered 55", dict(considered=(55, 4), noise=2, vo=256, scale=65), CONSIDERED_MSG),
    ("considered -1", dict(considered=(16, -1), n=1), CONSIDERED_MSG),
    ("gumbel_noise 2", dict(noise=2, vo=256, scale=65), b"gumbel_noise must be 0 or 1"),
    ("visit_offset 256", dict(vo=256, scale=65), b"visit_offset must be in [0, 255]"),
    ("scale 65", dict(scale=65, n=1), b"scale must be in [0, 64]"),
    ("state", dict(n=1), b"state must not be NULL"),
    ("to_move", dict(n=1, state=True), b"to_move must not be NULL"),
    ("done", dict(n=1, state=True, to_move=True), b"done must not be NULL"),
    ("an evaluator", dict(n=1, state=True, to_move=True, done=True, evs=(True, False)), b"ev must not be NULL"),
    ("no Gumbel side reads the three", dict(considered=(0, 0), noise=2, vo=-1, scale=65), None),
    ("a RANDOM side's bad values are ignored", dict(pols=("random", "eval"), deps=(7, 3), considered=(-5, 4), evs=(False, True)), None),
    ("... nor do they make the three read", dict(pols=("eval", "random"), considered=(0, 9), deps=(2, 99), scale=99, evs=(True, False)), None),
    ("the ends of the ranges", dict(considered=(54, 1), deps=(6, 0), noise=0, vo=255, scale=64), None),
]


@pytest.mark.parametrize("flavour", ["host", "device"])
def test_argument_errors(flavour):
    """(the device entry point checks its arguments before any HIP call: no GPU needed)"""
    lib, prefix = (nat.cpu_raw(), "gbl_cpu_") if flavour == "host" else (nat.lib(), "gbl_")
    err, f = getattr(lib, prefix + "last_error"), getattr(lib, prefix + "collect_gumbel_solve")
    net = smoke_net()
    boards = np.zeros((64, 27), np.int8)
    for name, over, msg in ERRORS:
        kw = dict(pols=("eval", "eval"), its=(8, 5), deps=(2, 3), considered=(16, 4), noise=1, vo=50, scale=23, n=0, state=False, to_move=False,
                  done=False, evs=(True, True))
        kw.update(over)
        evs = [net.struct() if e else None for e in kw["evs"]]
        st, tm, dn = (boards if kw[k] else None for k in ("state", "to_move", "done"))
        rc = f(*call_args(lambda a: None if a is None else a.ctypes.data, st, tm, dn, {}, kw["n"], 64, 64, 1, 0, 0, None, 4, kw["pols"], 16, 0,
                          nat.ILLEGAL_NOOP, None, None, None, evs, kw["its"], kw["deps"], kw["considered"], kw["noise"], kw["vo"], kw["scale"]))
        if msg is None:
            assert rc == nat.OK, (name, err())
        else:
            assert rc == nat.ERR_ARG and err() == msg, (name, rc, err())


def test_the_table_is_both_headers_declaration():
    """nat.SELFPLAY_ARGS_MORE against the declaration in include/gobblet_hip.h and include/gobblet_cpu.h, parameter by parameter: the
    name, and the ctype of its C type; and the arguments are gbl_collect_search_solve's followed, before `stream`, by
    gbl_collect_search_gumbel's five."""
    ctype_of = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}
    assert set(nat.SELFPLAY_ARGS_MORE) == {ENTRY} and not set(nat.SELFPLAY_ARGS_MORE) & set(nat.SELFPLAY_ARGS)
    table = nat.SELFPLAY_ARGS_MORE[ENTRY]
    for header, name in (("gobblet_hip.h", ENTRY), ("gobblet_cpu.h", "gbl_cpu_" + ENTRY[4:])):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        declared = []
        for param in re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M).group(1).split(","):
            ctype, pointer, param_name = re.fullmatch(r"\s*(?:const )?(\w+) (\*?)(\w+)\s*", param).groups()
            declared.append((param_name, C.c_void_p if pointer else ctype_of[ctype]))
        assert declared == list(table), (header, [(d, t) for d, t in zip(declared, table) if d != t], len(declared), len(table))
    assert nat.SIGNATURES[ENTRY] == (C.c_int, [t for _, t in table]) == nat.CPU_SIGNATURES["gbl_cpu_" + ENTRY[4:]]
    solve, gumbel = nat.SELFPLAY_ARGS["gbl_collect_search_solve"], nat.SELFPLAY_ARGS["gbl_collect_search_gumbel"]
    assert table == solve[:-1] + gumbel[-6:-1] + solve[-1:] and table[-1][0] == "stream"
    assert nat.selfplay_table(ENTRY) is table and nat.selfplay_table("gbl_collect_search") is nat.SELFPLAY_ARGS["gbl_collect_search"]
    with pytest.raises(TypeError, match="'scale'"):
        nat.selfplay_args(ENTRY, **{k: None for k, _ in table if k != "scale"})
    with pytest.raises(TypeError, match="'noise0'"):
        nat.selfplay_args(ENTRY, **{k: None for k, _ in table}, noise0=0)


def _collect(n, policies, search, seed=11, **kw):
    env = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, env_base=3, track_turn=True)
    env.rollout(64)
    env._lib = Counting(env._lib)
    return env.collect(4, policies=policies, search=search, out="fresh", **kw), env


def test_collect_surface(cpu, nets):
    net = nets[64]
    ev = _evaluator(net)
    base = dict(evaluator=ev, iterations=(8, 12), sample_plies=32, explore=24)
    # which entry point each spelling reaches
    for gumbel, entry in ((dict(considered=16), "gbl_collect_search_gumbel"), (dict(considered=16, solve_depth=0), "gbl_collect_search_gumbel"),
                          (dict(considered=16, solve_depth=(0, 0)), "gbl_collect_search_gumbel"),
                          (dict(considered=0, solve_depth=0), "gbl_collect_search_eval"),
                          (dict(considered=16, solve_depth=3), ENTRY), (dict(considered=(5, 0), solve_depth=(0, 2), scale=40, noise=True), ENTRY),
                          (dict(considered=0, solve_depth=2), ENTRY), (dict(solve_depth=(3, 0)), ENTRY)):
        tr, env = _collect(65, ("evaluator", "evaluator"), dict(base, gumbel=gumbel))
        assert set(env._lib.calls) == {entry}, (gumbel, env._lib.calls)
        assert ("outcomes" in tr and "proven" in tr) == (entry == ENTRY)
    tr, env = _collect(65, ("random", "evaluator"), dict(base, gumbel=dict(considered=(99, 4), solve_depth=(99, 0))))  # a random side's are dropped
    assert set(env._lib.calls) == {"gbl_collect_search_gumbel"} and "outcomes" not in tr
    # the new keys, and the window against the raw entry point
    got, env = _collect(65, ("evaluator", "evaluator"), dict(base, gumbel=dict(considered=(5, 0), solve_depth=(3, 2), scale=40, noise=True)))
    assert got["outcomes"].shape == (4, 65, 54) and got["outcomes"].dtype == torch.int8
    assert got["proven"].shape == (4, 65) and got["proven"].dtype == torch.int8
    ref = G.BatchedGobblet(65, "cpu", auto_reset=True, seed=11, env_base=3, track_turn=True)
    ref.rollout(64)
    raw = host_collect_gs(ref.squares.numpy(), ref.to_move.numpy(), ref.turn.numpy(), 4, ("eval", "eval"), (net, net), (8, 12), (3, 2), (5, 0),
                          1, 50, 40, 24, 32, nat.ILLEGAL_NOOP, "time", 11, 3, 64)[0]
    for k in raw:
        assert np.array_equal(got[k].numpy().reshape(raw[k].shape), raw[k]), k
    how = got["how"].numpy()
    assert {nat.HOW_PROVEN, nat.HOW_GUMBEL} <= set(np.unique(how).tolist()) and (how[got["mover"].numpy() == 1] != nat.HOW_GUMBEL).all()
    tile, _ = _collect(65, ("evaluator", "evaluator"), dict(base, gumbel=dict(solve_depth=2)), layout="tile")
    assert tile["outcomes"].shape == (2, 4, 64, 54)
    # every ValueError
    for bad in (dict(solve_depth=7), dict(solve_depth=-1), dict(solve_depth=(1, 2, 3)), dict(solve_depth=2.5), dict(solve_depth=True),
                dict(solve_depth=3, considered=55), dict(solve_depth=3, scale=65), dict(solve_depth=3, budget=1)):
        with pytest.raises(ValueError):
            _collect(8, ("evaluator", "evaluator"), dict(base, gumbel=bad))
    for other in (dict(solve_depth=2), dict(noise=0.25), dict(cap=dict(fast_iterations=2, full=0.25))):  # beside gumbel=: still refused
        with pytest.raises(ValueError, match="gumbel"):
            _collect(8, ("evaluator", "evaluator"), dict(base, gumbel=dict(solve_depth=3), **other))
    tb = G.Tablebase((1, 0, 0), "cpu")
    tb.build()
    env = G.BatchedGobblet(8, "cpu", auto_reset=True, seed=1, track_turn=True)
    with pytest.raises(ValueError, match="gumbel"):  # a "tablebase" side and the judge
        env.collect(3, policies=("tablebase", "evaluator"), search=dict(tablebase=tb, evaluator=ev, iterations=8, gumbel=dict(solve_depth=3)))
    with pytest.raises(ValueError, match="gumbel"):
        env.collect(3, policies=("evaluator", "evaluator"), search=dict(tablebase=tb, judge=True, evaluator=ev, iterations=8, gumbel=dict(solve_depth=3)))
    # the single decision and reanalysis: solve_depth stays an unknown key there, and the message names the policy that composes it
    with pytest.raises(ValueError, match="SolverGobbletPolicy"):
        G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=16, gumbel=dict(solve_depth=3), device="cpu")
    from gobblet_rl_amd.evaluator_policy import gumbel_args
    with pytest.raises(ValueError, match="SolverGobbletPolicy"):
        gumbel_args(dict(considered=16, solve_depth=0))
