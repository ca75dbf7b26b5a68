"""gbl_collect_search / gbl_outcome_targets on the MI355X (-m gpu): k_collect_search against the Python restatement of the contract,
against the host flavour and against the composed loop of gbl_tree_search + gbl_step_into, k_outcome_targets against the host
flavour, a graph capture, a performance guard on the committed record (profiles/r09/selfplay_search.json, written by
scripts/bench_selfplay_search.py) and the fused launch against the composed loop in one process."""
import json
import os
import statistics
import sys

import numpy as np
import pytest
import torch

from tests import selfplay_harness as H
from tests.search_harness import G, midgame_boards  # noqa: F401  (G: the fixture)
from tests.selfplay_harness import DEV, same
from tests.test_selfplay_search import GRID, collect, restate_collect

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


@pytest.fixture(scope="module")
def c5(G):
    return midgame_boards(turn=True)


# gbl_collect_search on the device (H.device_collect) under the argument order of tests.test_selfplay_search.collect
device_collect = lambda G, st, tm, turn, T, pols, its, pls, M, X, *a, **kw: H.device_collect(  # noqa: E731
    "search", st, tm, turn, T, pols, X, *a, its=its, pls=pls, M=M, **kw)


@pytest.mark.parametrize("pols,its,pls,sample_plies,illegal_mode,ply_dev", GRID)
def test_device_equals_restatement(G, c5, pols, its, pls, sample_plies, illegal_mode, ply_dev):
    st = np.concatenate([np.zeros((2, 27), np.int8), c5[0][:10]])
    tm = np.concatenate([np.zeros(2, np.int8), c5[1][:10]])
    turn = np.concatenate([np.zeros(2, np.int32), c5[2][:10] % 7])  # (some of them inside the sampled plies)
    M, X, seed, env_base, ply0, T = 40, 128, 9, (1 << 40) - 20, 5, 12
    exp = restate_collect(st, tm, turn, T, pols, its, pls, M, X, sample_plies, illegal_mode, seed, env_base, ply0 + (ply_dev or 0))
    for layout in ("time", "tile"):
        same(device_collect(G, st, tm, turn, T, pols, its, pls, M, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, ply_dev), exp)


# (64 iterations of 16 playouts run k_collect_search<1>; 256 playouts <4> up to 1 024 boards, <2> up to 2 048)
@pytest.mark.parametrize("n", [1, 63, 64, 257, 4096])
def test_device_equals_host_flavour(G, c5, n):
    st, tm, turn = c5[0][:n], c5[1][:n], c5[2][:n] % 9
    cpu = G._native.cpu_raw()
    for layout in ("time", "tile"):
        args = (8, ("tree", "tree"), (64, 64), (16, 16), 64, 16, 3, 0, layout, 3, 17, 4)
        same(device_collect(G, st, tm, turn, *args), collect(cpu, st, tm, turn, *args))
    if n <= 257:  # the wider workgroups, unequal sides, a random side, the other illegal mode
        args = (5, ("tree", "tree"), (20, 12), (256, 130), 30, 128, 2, 1, "time", 1, 0, 0, 7)
        same(device_collect(G, st, tm, turn, *args), collect(cpu, st, tm, turn, *args))
        args = (6, ("random", "tree"), (0, 300), (0, 6), 64, 64, 0, 0, "tile", 1, 0, 0)
        same(device_collect(G, st, tm, None, *args), collect(cpu, st, tm, None, *args))


def test_device_equals_host_flavour_config5_full_size(G, c5):
    st, tm, turn = c5
    args = (2, ("tree", "tree"), (48, 48), (4, 4), 64, 128, 0, 0, "time", 0, 0, 0)
    same(device_collect(G, st, tm, turn, *args), collect(G._native.cpu_raw(), st, tm, turn, *args))


def test_device_equals_composed_loop(G, c5):
    import bench_selfplay_search as B
    r = B.Runner(torch.from_numpy(c5[0][:4096]).to(DEV), torch.from_numpy(c5[1][:4096]).to(DEV), 64, 16, plies=6, seed=5)
    r.check_equal()


def test_outcome_targets_device_equals_host_flavour(G):
    nat = G._native
    n, T = 65536, 32
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=2, track_turn=True)
    for layout in ("time", "tile"):
        out = env.collect(T, out=env.trajectory_buffers(T, layout=layout, search_outputs=True, placement="any"), policies=("tree", "random"),
                          search=dict(iterations=16, playouts=4, max_plies=32, sample_plies=2))
        env.outcome_targets(out)
        torch.cuda.synchronize()
        f = {k: v.cpu().numpy() for k, v in out["_full"].items() if k in ("done", "rewards", "mover", "z", "plies_left")}
        assert f["done"].sum() > n // 4  # (the searching side finishes games)
        z, left = np.full_like(f["z"], nat.Z_OPEN), np.full_like(f["plies_left"], -1)
        rc = nat.cpu_raw().gbl_cpu_outcome_targets(f["done"].ctypes.data, f["rewards"].ctypes.data, f["mover"].ctypes.data, z.ctypes.data,
                                                  left.ctypes.data, n, out["_ply_stride"], out["_tile_stride"], T, None)
        assert rc == 0
        assert np.array_equal(f["z"], z) and np.array_equal(f["plies_left"], left)
        assert (z == 1).any() and (z == -1).any() and (z == nat.Z_OPEN).any()


def test_graph_capture_draws_afresh(G, c5):
    """One captured collect(..., search=...) + advance_ply(): a single linear chain; every replay searches with new call indices."""
    n, T = 2048, 3
    kw = dict(policies=("tree", "tree"), search=dict(iterations=32, playouts=8, max_plies=40, sample_plies=2))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=7, track_turn=True)
    env.rollout(3)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T, search_outputs=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    seen = []
    with torch.cuda.stream(side):
        env.collect(T, out=buf, **kw); env.advance_ply()  # warm-up on the side stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            env.collect(T, out=buf, **kw)
            env.advance_ply()
        for _ in range(2):
            g.replay()
            side.synchronize()
            seen.append({k: buf[k].clone() for k in ("actions", "visits", "value", "how", "mover", "observation")})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert env.ply == 3 + 3 * T
    ref = G.BatchedGobblet(n, DEV, auto_reset=True, seed=7, track_turn=True)
    ref.load_state_dict(sd)
    for r in range(3):  # the eager launch and the two replays, as three eager launches
        out = ref.collect(T, out="fresh", **kw)
        if r:
            assert all(torch.equal(out[k], seen[r - 1][k]) for k in seen[0]), r
    assert torch.equal(env.squares, ref.squares) and torch.equal(env.turn, ref.turn)
    assert not torch.equal(seen[0]["visits"], seen[1]["visits"])


# ceilings: the committed record + 15 % (boxes differ by a few percent; HIP-event medians)
RECORD = os.path.join(ROOT, "profiles", "r09", "selfplay_search.json")


@pytest.mark.parametrize("n,I,P", [(4096, 64, 16), (65536, 64, 16)])
def test_selfplay_perf_guard(G, c5, n, I, P):
    import bench_selfplay_search as B
    rec = {(r["boards"], r["iterations"], r["playouts"]): r for r in json.load(open(RECORD))["rows"]}[(n, I, P)]
    r = B.Runner(torch.from_numpy(c5[0][:n]).to(DEV), torch.from_numpy(c5[1][:n]).to(DEV), I, P, plies=rec["plies"])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(6):
        r.restore()
        torch.cuda.synchronize()
        e0.record()
        r.fused()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print("fused ms", ms, "record", rec["fused_ms"])
    assert statistics.median(ms[1:]) <= 1.15 * rec["fused_ms"]["median"], (ms, rec["fused_ms"])


def test_fused_is_not_slower_than_composed(G, c5):
    """(a) one gbl_collect_search launch against (b) the loop of gbl_tree_search + gbl_step_into, in one process, 4 096 boards,
    (64, 16), 16 plies: (a) does strictly less, so its median must not exceed (b)'s by more than (b)'s own min-to-max spread.
    Measured (profiles/r09/selfplay_search.json): fused 25.22 ms (25.19 - 25.25), composed 31.21 ms (31.17 - 31.29), ratio 0.808."""
    import bench_selfplay_search as B
    r = B.Runner(torch.from_numpy(c5[0][:4096]).to(DEV), torch.from_numpy(c5[1][:4096]).to(DEV), 64, 16)
    a, b = r.time()
    print("fused ms", a, "composed ms", b)
    assert B.within_spread(a, b), (a, b)
