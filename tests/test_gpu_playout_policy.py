"""gbl_playout_values on the MI355X (-m gpu): k_playout against the Python restatement of the contract and against the host
flavour, the arena on both, and a performance guard on the committed record (profiles/r07/playout_policy.json, written by
scripts/bench_playout_policy.py)."""
import json
import os
import statistics

import numpy as np
import pytest
import torch

import oracle
from tests.search_harness import DEV, Call, G, midgame_boards, run, same  # noqa: F401  (G: the fixture)
from tests.test_playout_policy import arena, restate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def c5(G):
    return midgame_boards()


@pytest.mark.parametrize("K,M,call,env_base", [(7, 30, 5, (1 << 40) - 20), (3, 255, 0, 0), (5, 0, 2, 11)])
def test_device_equals_restatement(G, c5, K, M, call, env_base):
    st, tm = c5[0][:6], c5[1][:6]
    st = np.concatenate([np.zeros((1, 27), np.int8), st])
    tm = np.concatenate([np.zeros(1, np.int8), tm])
    mask = None if K != 3 else (np.random.default_rng(1).random((len(st), 54)) < 0.5).astype(np.int8)
    same(run("playout_values", DEV, st, tm, mask, (K, M, 9, env_base, call)), restate(st, tm, mask, K, M, 9, env_base, call))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4096])
def test_device_equals_host_flavour(G, c5, n):
    st, tm = c5[0][:n], c5[1][:n]
    same(run("playout_values", DEV, st, tm, None, (64, 64, 3, 17, 4)), run("playout_values", "cpu", st, tm, None, (64, 64, 3, 17, 4)))
    mask = (np.random.default_rng(n).random((n, 54)) < 0.3).astype(np.int8)
    same(run("playout_values", DEV, st, tm, mask, (64, 64, 3, 17, 4)), run("playout_values", "cpu", st, tm, mask, (64, 64, 3, 17, 4)))


def test_device_equals_host_flavour_config5_full_size(G, c5):
    st, tm = c5
    same(run("playout_values", DEV, st, tm, None, (4, 64, 0, 0, 0)), run("playout_values", "cpu", st, tm, None, (4, 64, 0, 0, 0)))


def test_arena_device_equals_host_flavour(G):
    gpu = arena(G.MonteCarloGobbletPolicy(playouts=16, max_plies=64, seed=0, device=DEV), 512, seed=7)
    cpu = arena(G.MonteCarloGobbletPolicy(playouts=16, max_plies=64, seed=0, device="cpu"), 512, seed=7)
    assert gpu == cpu and gpu >= 0.85 * 512
    gpu = arena(G.MonteCarloGobbletPolicy(playouts=16, max_plies=64, seed=0, device=DEV), 256, seed=7, opponent="greedy")
    cpu = arena(G.MonteCarloGobbletPolicy(playouts=16, max_plies=64, seed=0, device="cpu"), 256, seed=7, opponent="greedy")
    assert gpu == cpu


def test_policy_on_device(G, c5):
    st, tm = torch.from_numpy(c5[0][:256]).to(DEV), torch.from_numpy(c5[1][:256]).to(DEV)
    pol = G.MonteCarloGobbletPolicy(playouts=32, seed=5, device=DEV)
    v = pol.action_values(st, tm)
    exp = run("playout_values", "cpu", c5[0][:256], c5[1][:256], None, (32, 64, 5, 0, 0))
    assert pol.last_wins.device.type == "cuda" and np.array_equal(pol.last_wins.cpu().numpy(), exp["wins"])
    assert np.array_equal(pol.last_action.cpu().numpy(), exp["action"]) and np.array_equal(pol.last_plies.cpu().numpy(), exp["plies"])
    assert torch.isfinite(v).sum() == int((oracle.batch_legal_mask(c5[0][:256], c5[1][:256]) != 0).sum())


# ceilings: the committed record + 15 % (boxes differ by a few percent; HIP-event medians)
RECORD = os.path.join(ROOT, "profiles", "r07", "playout_policy.json")


@pytest.mark.parametrize("n,K", [(4096, 64), (65536, 64), (65536, 16)])
def test_playout_perf_guard(G, c5, n, K):
    rec = {(r["boards"], r["playouts"]): r for r in json.load(open(RECORD))["rows"]}[(n, K)]
    launch = Call("playout_values", DEV).load(c5[0][:n], c5[1][:n]).launch

    def go(call):
        launch((K, 64, 0, 0, call))
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
