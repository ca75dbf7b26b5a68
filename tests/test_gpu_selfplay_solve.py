"""gbl_collect_search_solve on the MI355X (-m gpu): k_collect_solve against the host flavour, bit for bit and with canaries of 16
elements around every output, at the batch sizes of cell()'s tile edge; depth 4 (the deepest the phase-2 deal is affordable at in a
test); 512 iterations beside the solver's LDS arrays; against the Python restatement of the contract; NULL optional outputs; a batch
beyond the grid cap; a graph capture and replay; BatchedGobblet.collect(solve_depth=) against the same on "cpu"; and the two
performance guards of the record profiles/r16/selfplay_solve.json."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import evaluator_restatement as R
from tests import solver_restatement as SR
from tests import selfplay_harness as H
from tests.search_harness import G, run  # noqa: F401  (G: the fixture)
from tests.selfplay_harness import DEV, DeviceNet, _evaluator, same
from tests.test_selfplay_solve import CASES, EXPLORE, T, WINDOW, collect_solve, fixture_boards, restated_six, six_boards, smoke_net

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_CAP = 1 << 20


@pytest.fixture(scope="module")
def c5(G):
    return fixture_boards(65536, DEV)


@pytest.fixture(scope="module")
def nets(G):
    """(host nets, device nets): smoke()'s network and a second one of another width."""
    pair = (smoke_net(), R.random_net(128, 77))
    return pair, tuple(DeviceNet(x) for x in pair)


def host_collect(G, *args, **kw):
    cpu = G._native.cpu_raw()
    return collect_solve(cpu.gbl_cpu_collect_search_solve, cpu.gbl_cpu_last_error, *args, **kw)


# gbl_collect_search_solve on the device, every output between canaries (H.device_collect), under collect_solve's argument order
device_collect = lambda G, st, tm, turn, T_, pols, dnets, its, deps, X, *a, **kw: H.device_collect("solve", st, tm, turn, T_, pols, X, *a, nets=dnets, its=its, deps=deps, **kw)  # noqa: E731


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257])
def test_device_equals_host_flavour(G, c5, nets, n):
    hn, dn = nets
    st, tm, turn = c5[0][:n], c5[1][:n], c5[2][:n] % 5
    for deps, layout, sp, mode in (((2, 3), "time", 2, 0), ((2, 3), "tile", 0, 1), ((3, 0), "time", 0, 1), ((3, 0), "tile", 2, 0)):
        args = ((8, 3), deps, EXPLORE, sp, mode, layout, 3, 17, 4)
        got = device_collect(G, st, tm, turn, T, ("eval", "eval"), dn, *args)
        same(got, host_collect(G, st, tm, turn, T, ("eval", "eval"), hn, *args))
    # a random side, NULL for its evaluator, its depth not read, the ply index through ply_dev
    args = ((0, 8), (9, 3), 16, 2, 0, "time", 1, 0, 0, 7)
    same(device_collect(G, st, tm, turn, T, ("random", "eval"), (None, dn[1]), *args),
         host_collect(G, st, tm, turn, T, ("random", "eval"), (None, hn[1]), *args))
    if n >= 63:
        how = got[0]["how"]
        assert (how == G._native.HOW_PROVEN).any() and (how == G._native.HOW_SEARCH).any()


def test_depth_4(G, c5, nets):
    """3 boards x 2 plies: the phase-2 deal with two plies below every pair."""
    hn, dn = nets
    st, tm, turn = c5[0][:3], c5[1][:3], c5[2][:3]
    args = (2, ("eval", "eval"), None, (8, 8), (4, 4), EXPLORE, 0, 0, "time", 1, 0, 0)
    got = device_collect(G, st, tm, turn, *args[:2], dn, *args[3:])
    same(got, host_collect(G, st, tm, turn, *args[:2], hn, *args[3:]))
    assert (got[0]["outcomes"] != SR.NONE).any()


def test_512_iterations_beside_the_solver(G, c5, nets):
    """The LDS limit of the tree (36.9 KB) beside the solver's arrays: 3 boards, 2 plies, depth 2."""
    hn, dn = nets
    # boards whose first roots are unproven at depth 2, so that the 512 iterations run
    out = run("solve", "cpu", c5[0][:64], c5[1][:64], None, (2,))
    pick = np.flatnonzero(out["value"] == 0)[:3]
    st, tm, turn = c5[0][pick], c5[1][pick], c5[2][pick]
    args = (2, ("eval", "eval"), None, (512, 512), (2, 2), 64, 0, 0, "time", 1, 0, 0)
    got = device_collect(G, st, tm, turn, *args[:2], dn, *args[3:])
    same(got, host_collect(G, st, tm, turn, *args[:2], hn, *args[3:]))
    assert (got[0]["visits"].sum(2) == 512).all() and (got[0]["nodes"][0] > 1).all() and (got[0]["nodes"] <= 513).all()


@pytest.mark.parametrize("case,sample_plies,illegal_mode", [(0, 2, 0), (1, 0, 1), (2, 2, 1), (3, 0, 0)])
def test_device_equals_restatement(G, c5, case, sample_plies, illegal_mode):
    pols, deps, its = CASES[case]
    st, tm, turn = six_boards(c5)
    net = smoke_net()
    dnet = DeviceNet(net)
    use = tuple(dnet if p == "eval" else None for p in pols)
    exp = restated_six(case, sample_plies, illegal_mode)
    for layout in ("time", "tile"):
        same(device_collect(G, st, tm, turn, T, pols, use, its, deps, EXPLORE, sample_plies, illegal_mode, layout, WINDOW["seed"],
                            WINDOW["env_base"], WINDOW["ply0"] - 3, 3), exp)


def test_null_optional_outputs(G, c5, nets):
    hn, dn = nets
    st, tm, turn = c5[0][:130], c5[1][:130], c5[2][:130] % 3
    args = (3, ("eval", "eval"), dn, (8, 4), (2, 3), 64, 2, 0, "time", 3, 0, 0)
    full = device_collect(G, st, tm, turn, *args)
    for keep in (("actions",), ("outcomes",), ("proven",), ("visits", "root_value", "proven"), ("priors", "outcomes"),
                 ("value", "nodes", "how", "mover", "observation"), ("action_mask", "outcomes", "proven"), ()):
        got = device_collect(G, st, tm, turn, *args, keep=keep)
        assert set(got[0]) == set(keep)
        same(got, full)


def test_beyond_the_grid_cap(G, c5, nets):
    """2^20 + 65 boards, one ply, depth 1, one iteration: the grid-stride loop's second trip must keep nothing of the first trip's
    solve."""
    hn, dn = nets
    n = GRID_CAP + 65
    st, tm, turn = np.resize(c5[0], (n, 27)), np.resize(c5[1], n), np.resize(c5[2] % 3, n)
    keep = ("actions", "visits", "how", "outcomes", "proven")
    # (env_base 0 and sample_plies 0: a searching board's ply depends on the board alone, so the batch repeats its head)
    args = (1, ("eval", "eval"), None, (1, 1), (1, 1), 64, 0, 0, "tile", 3, 0, 0)
    got = device_collect(G, st, tm, turn, *args[:2], dn, *args[3:], keep=keep)
    head = host_collect(G, st[:65536], tm[:65536], turn[:65536], *args[:2], hn, *args[3:], keep=keep)
    for k in keep:
        assert np.array_equal(got[0][k], head[0][k][:, np.arange(n) % 65536]), k
    assert np.array_equal(got[1], np.resize(head[1], (n, 27))) and np.array_equal(got[4], np.resize(head[4], n))


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "outcomes", "proven", "observation", "done")


def test_graph_capture_and_replay(G):
    """One captured guarded launch with ply_dev, replayed twice (gbl_counter_add advances the ply inside the graph): the same as two
    eager launches."""
    n, T_, seed = 300, 3, 7
    ev = _evaluator(smoke_net(), DEV)
    kw = dict(policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=8, solve_depth=(2, 3), sample_plies=2))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    env.rollout(20)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T_, search_outputs=True, evaluator_outputs=True, solver_outputs=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    seen = []
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            env.collect(T_, out=buf, **kw)
            env.advance_ply()
        for i in range(2):
            g.replay()
            side.synchronize()
            seen.append({k: buf[k].clone() for k in KEYS})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    ref.load_state_dict(sd)
    for i in range(2):
        out = ref.collect(T_, out="fresh", **kw)
        for k in KEYS:
            assert torch.equal(out[k], seen[i][k]), (i, k)
    assert torch.equal(env.squares, ref.squares) and torch.equal(env.turn, ref.turn)
    assert (seen[0]["how"] == G._native.HOW_PROVEN).any() and not torch.equal(seen[0]["actions"], seen[1]["actions"])


def test_collect_with_solve_depth_equals_cpu(G):
    net = smoke_net()
    outs = []
    for d in (DEV, "cpu"):
        env = G.BatchedGobblet(200, d, auto_reset=True, seed=11, env_base=3, track_turn=True)
        env.rollout(30)
        out = env.collect(4, policies=("evaluator", "evaluator"), count=True,
                          search=dict(evaluator=_evaluator(net, d), iterations=(8, 5), solve_depth=(3, 2), sample_plies=40, explore=24))
        env.outcome_targets(out)
        outs.append((out, env))
    torch.cuda.synchronize()
    (a, ea), (b, eb) = outs
    for k in KEYS + ("z", "plies_left", "action_mask", "winner", "rewards", "to_move"):
        assert torch.equal(a[k].cpu(), b[k]), k
    assert torch.equal(ea.squares.cpu(), eb.squares) and torch.equal(ea.turn.cpu(), eb.turn) and int(ea.counters[0]) == 800
    assert (a["how"] == G._native.HOW_PROVEN).any() and (a["how"] == G._native.HOW_SEARCH_SAMPLED).any()
    batch = ea.training_batch(a, 256, call=2)
    assert (batch["visits"].sum(1)[batch["index"][:, 0] >= 0] > 0).all()


# ---- the guards of the record ------------------------------------------------------------------------------------------------------
def _bench():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import bench_selfplay_solve as B
    return B


def test_fused_4096_boards_depth_3_within_the_record(G):
    """4 096 boards x 64 iterations x H 64 x depth 3, 8 plies: the record's median (profiles/r16/selfplay_solve.json, section
    `guard`) plus 15 %, the margin the other guards use."""
    B = _bench()
    with open(os.path.join(ROOT, "profiles", "r16", "selfplay_solve.json")) as f:
        record = json.load(f)["guard"]["fused_ms"]["median"]
    r = B.Runner(*B.states(4096), 64, B.seeded_evaluator(64), 3, plies=8)
    ms = B.stats(r.time(reps=3, names=("fused",))["fused"])["median"]
    print("gbl_collect_search_solve 4096 boards x 8 plies, depth 3: %.3f ms (record %.3f)" % (ms, record))
    assert ms <= 1.15 * record, (ms, record)


def test_fused_no_slower_than_the_composed_loop(G):
    """In one process: the fused launch's median against the composed device loop's (gbl_solve + gbl_tree_search_eval(mask) +
    gbl_step_into) from the same position; the margin is the width of the composed loop's own min-max band in this run."""
    B = _bench()
    r = B.Runner(*B.states(4096), 64, B.seeded_evaluator(64), 3, plies=8)
    r.check_equal()
    t = r.time(reps=3)
    print("fused %s  composed %s" % (B.stats(t["fused"]), B.stats(t["composed"])))
    assert B.within_spread(t["fused"], t["composed"])
