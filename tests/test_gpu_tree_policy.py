"""gbl_tree_search on the MI355X (-m gpu): k_tree against the Python restatement of the contract and against the host flavour,
the arena on both, the policy on the device, and a performance guard on the committed record (profiles/r08/tree_policy.json,
written by scripts/bench_tree_policy.py)."""
import json
import os
import statistics

import numpy as np
import pytest
import torch

from tests.search_harness import DEV, Call, G, midgame_boards, run, same  # noqa: F401  (G: the fixture)
from tests.test_playout_policy import arena
from tests.test_tree_policy import restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c5(G):
    return midgame_boards()


@pytest.mark.parametrize("I,P,M,X,call,env_base", [(64, 4, 30, 128, 5, (1 << 40) - 20), (40, 3, 255, 0, 0, 0), (30, 130, 6, 1024, 2, 11)])
def test_device_equals_restatement(G, c5, I, P, M, X, call, env_base):
    st, tm = c5[0][:6], c5[1][:6]
    st = np.concatenate([np.zeros((1, 27), np.int8), st])
    tm = np.concatenate([np.zeros(1, np.int8), tm])
    mask = None
    if P == 3:
        mask = (np.random.default_rng(1).random((len(st), 54)) < 0.5).astype(np.int8)
        mask[2] = 0  # a board without a candidate
    same(run("tree_search", DEV, st, tm, mask, (I, P, M, X, 9, env_base, call)), restate(st, tm, mask, I, P, M, X, 9, env_base, call))


# (iterations, playouts): 256 playouts run k_tree<4> up to 1 024 boards, <2> up to 2 048 and <1> beyond; 600 iterations are a
# 9.6 KB tree, 40 one of 656 bytes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2000, 4096])
def test_device_equals_host_flavour(G, c5, n):
    st, tm = c5[0][:n], c5[1][:n]
    same(run("tree_search", DEV, st, tm, None, (40, 256, 64, 128, 3, 17, 4)), run("tree_search", "cpu", st, tm, None, (40, 256, 64, 128, 3, 17, 4)))
    mask = (np.random.default_rng(n).random((n, 54)) < 0.3).astype(np.int8)
    same(run("tree_search", DEV, st, tm, mask, (600, 6, 64, 64, 3, 17, 4)), run("tree_search", "cpu", st, tm, mask, (600, 6, 64, 64, 3, 17, 4)))
    if n <= 65:  # the largest tree
        same(run("tree_search", DEV, st, tm, None, (1024, 2, 20, 256, 1, 0, 0)), run("tree_search", "cpu", st, tm, None, (1024, 2, 20, 256, 1, 0, 0)))


def test_device_equals_host_flavour_config5_full_size(G, c5):
    st, tm = c5
    same(run("tree_search", DEV, st, tm, None, (48, 4, 64, 128, 0, 0, 0)), run("tree_search", "cpu", st, tm, None, (48, 4, 64, 128, 0, 0, 0)))


def test_arena_device_equals_host_flavour(G):
    kw = dict(iterations=64, playouts=8, max_plies=64, seed=0)
    gpu = arena(G.TreeSearchGobbletPolicy(device=DEV, **kw), 512, seed=7)
    cpu = arena(G.TreeSearchGobbletPolicy(device="cpu", **kw), 512, seed=7)
    assert gpu == cpu and gpu >= 0.85 * 512
    gpu = arena(G.TreeSearchGobbletPolicy(device=DEV, **kw), 256, seed=7, opponent="greedy")
    cpu = arena(G.TreeSearchGobbletPolicy(device="cpu", **kw), 256, seed=7, opponent="greedy")
    assert gpu == cpu


def test_policy_on_device(G, c5):
    st, tm = torch.from_numpy(c5[0][:256]).to(DEV), torch.from_numpy(c5[1][:256]).to(DEV)
    pol = G.TreeSearchGobbletPolicy(iterations=100, playouts=8, seed=5, device=DEV)
    val = pol.action_values(st, tm)
    exp = run("tree_search", "cpu", c5[0][:256], c5[1][:256], None, (100, 8, 64, pol.explore, 5, 0, 0))
    last = (pol.last_visits, pol.last_wins, pol.last_losses, pol.last_action, pol.last_nodes, pol.last_plies)
    assert all(t.device.type == "cuda" for t in last) and val.device.type == "cuda"
    same(exp, [t.cpu().numpy() for t in last])
    assert int(torch.isfinite(val).sum()) == int((exp["visits"] > 0).sum())
    dist = pol.visit_distribution(st, tm)
    exp1 = run("tree_search", "cpu", c5[0][:256], c5[1][:256], None, (100, 8, 64, pol.explore, 5, 0, 1))
    assert dist.device.type == "cuda" and np.array_equal(pol.last_visits.cpu().numpy(), exp1["visits"])
    assert np.allclose(dist.cpu().numpy(), exp1["visits"] / 100.0, rtol=1e-6, atol=0)  # (one float32 division: 2^-24 relative)


# ceilings: the committed record + 15 % (boxes differ by a few percent; HIP-event medians)
RECORD = os.path.join(ROOT, "profiles", "r08", "tree_policy.json")


@pytest.mark.parametrize("n,I,P", [(4096, 256, 16), (65536, 64, 16), (65536, 256, 64)])
def test_tree_perf_guard(G, c5, n, I, P):
    rec = {(r["boards"], r["iterations"], r["playouts"]): r for r in json.load(open(RECORD))["rows"]}[(n, I, P)]
    launch = Call("tree_search", DEV).load(c5[0][:n], c5[1][:n]).launch

    def go(call):
        launch((I, P, 64, rec["explore"], 0, 0, call))
    go(0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(5):
        e0.record()
        go(1 + i)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert statistics.median(ms) <= 1.15 * rec["ms_per_launch"], (ms, rec["ms_per_launch"])
