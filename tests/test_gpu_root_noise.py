"""Root noise on the MI355X (-m gpu): gbl_tree_search_eval_noise and gbl_collect_search_noise against the host flavour, bit for bit
and between canaries; NULL optional outputs; weights (0, 0) against gbl_collect_search_solve on the device; and one graph capture and
replay of collect(..., noise=) with the ply on the device.  The launches go through the launchers of gbl_tree_search_eval and
gbl_collect_search_solve (one grid rule, covered beyond its cap by tests/test_gpu_evaluator_policy.py and
tests/test_gpu_selfplay_solve.py), so no case beyond the grid cap is repeated here."""
import numpy as np
import pytest
import torch

import oracle

from tests import evaluator_restatement as R
from tests import selfplay_harness as H
from tests.search_harness import DEV, G, run  # noqa: F401  (G: the fixture)
from tests.search_harness import same as same_arrays
from tests.selfplay_harness import DeviceNet, _evaluator, same
from tests.test_selfplay_solve import EXPLORE, collect_solve, fixture_boards, smoke_net

pytestmark = pytest.mark.gpu

SEED, ENV_BASE, CALL = 0x1234567890ABCDEF, (1 << 40) + 3, (1 << 24) - 1


@pytest.fixture(scope="module")
def c5(G):
    return fixture_boards(256, DEV)


@pytest.mark.parametrize("iterations", [1, 8, 64])
@pytest.mark.parametrize("hidden", [64, 256])
def test_k_tree_eval_noise_equals_host_flavour(G, c5, hidden, iterations):
    net = R.random_net(hidden, 5 + hidden)
    dnet = DeviceNet(net)
    for n in (1, 5, 65):
        st, tm = c5[0][:n], c5[1][:n]
        for w in (0, 1, 64, 256):
            args = (st, tm, None, (iterations, EXPLORE, w, SEED, ENV_BASE, CALL if w != 64 else 0))
            got = run("tree_search_eval_noise", DEV, *args, dnet)
            same_arrays(got, run("tree_search_eval_noise", "cpu", *args, net))
            if w == 0:
                assert np.array_equal(got["root_mixed"], got["root_priors"])


def test_masked_roots_and_null_outputs(G, c5):
    net = R.random_net(128, 1)
    dnet = DeviceNet(net)
    st, tm = c5[0][:70], c5[1][:70]
    legal = oracle.batch_legal_mask(st, tm)
    mask = (np.random.default_rng(6).random((70, 54)) < 0.4).astype(np.int8)
    mask[0] = 0  # no candidate: nothing is drawn, the rows stay zeros
    mask[1] = 0
    mask[1, np.flatnonzero(legal[1])[3]] = 1  # one candidate: nu = 255, and so is pi
    args = (st, tm, mask, (24, EXPLORE, 128, SEED, 7, 5))
    full = run("tree_search_eval_noise", DEV, *args, dnet)
    same_arrays(full, run("tree_search_eval_noise", "cpu", *args, net))
    assert not full["root_mixed"][0].any() and full["action"][0] == -1 and full["nodes"][0] == 1
    assert full["root_mixed"][1].max() == 255 and (full["root_mixed"][1] > 0).sum() == 1
    for keep in (("action",), ("root_mixed",), ("visits", "root_priors"), ("wins", "losses", "nodes", "root_value"), ()):
        got = run("tree_search_eval_noise", DEV, *args, dnet, keep)
        assert set(got) == set(keep)
        same_arrays(got, full)


# ---- self-play -----------------------------------------------------------------------------------------------------------------------
def host_collect(G, noise, *args, **kw):
    cpu = G._native.cpu_raw()
    f = cpu.gbl_cpu_collect_search_solve if noise is None else cpu.gbl_cpu_collect_search_noise
    return collect_solve(f, cpu.gbl_cpu_last_error, *args, noise=noise, **kw)


# gbl_collect_search_noise (noise None: gbl_collect_search_solve) on the device, every output between canaries (H.device_collect)
device_collect = lambda G, noise, st, tm, turn, T_, pols, dnets, its, deps, X, *a, **kw: H.device_collect(  # noqa: E731
    "solve" if noise is None else "noise", st, tm, turn, T_, pols, X, *a, nets=dnets, its=its, deps=deps, noise=noise or (0, 0), **kw)


@pytest.fixture(scope="module")
def nets(G):
    """(host nets, device nets): smoke()'s network and a second one of another width."""
    pair = (smoke_net(), R.random_net(128, 77))
    return pair, tuple(DeviceNet(x) for x in pair)


@pytest.mark.parametrize("n", [5, 65])
def test_k_collect_noise_equals_host_flavour(G, c5, nets, n):
    hn, dn = nets
    st, tm, turn = c5[0][:n], c5[1][:n], c5[2][:n] % 5
    for deps, layout, sp in (((0, 0), "time", 2), ((2, 0), "tile", 0), ((3, 3), "time", 2)):
        for noise in ((64, 0), (64, 256)):
            args = (st, tm, turn, 6, ("eval", "eval"), None, (8, 3), deps, EXPLORE, sp, 0, layout, 3, ENV_BASE, 4)
            got = device_collect(G, noise, *args[:5], dn, *args[6:])
            same(got, host_collect(G, noise, *args[:5], hn, *args[6:]))
        # weights (0, 0): the guarded launch itself, on the device
        args = (st, tm, turn, 6, ("eval", "eval"), dn, (8, 3), deps, EXPLORE, sp, 0, layout, 3, ENV_BASE, 4)
        same(device_collect(G, (0, 0), *args), device_collect(G, None, *args))
    if n == 65:
        how = got[0]["how"]
        assert (how == G._native.HOW_PROVEN).any() and (how == G._native.HOW_SEARCH).any()
    # a random side: its weight is not read (a value outside the range), the ply index through ply_dev
    args = (st, tm, turn, 6, ("random", "eval"), None, (0, 8), (9, 2), 16, 2, 0, "time", 1, 0, 0, 7)
    same(device_collect(G, (999, 128), *args[:5], (None, dn[1]), *args[6:]), host_collect(G, (-5, 128), *args[:5], (None, hn[1]), *args[6:]))


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "outcomes", "proven", "observation", "done")


def test_graph_capture_and_replay(G):
    """One captured noised launch with ply_dev, replayed twice (gbl_counter_add advances the ply inside the graph): every replay equals
    the HOST flavour's window at the advanced ply, so the noise moves with *ply_dev."""
    n, T_, seed = 130, 3, 7
    net = smoke_net()
    kw = lambda d: dict(policies=("evaluator", "evaluator"),  # noqa: E731
                        search=dict(evaluator=_evaluator(net, d), iterations=8, solve_depth=(2, 0), sample_plies=2, noise=(0.25, 1.0)))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    env.rollout(20)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T_, search_outputs=True, evaluator_outputs=True, solver_outputs=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    seen = []
    kd = kw(DEV)
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            env.collect(T_, out=buf, **kd)
            env.advance_ply()
        for i in range(2):
            g.replay()
            side.synchronize()
            seen.append({k: buf[k].clone() for k in KEYS})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, track_turn=True)
    ref.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})
    kc = kw("cpu")
    plain = None
    for i in range(2):
        if i == 0:  # the same window without noise, from the same state: the noise changed what was played
            twin = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, track_turn=True)
            twin.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})
            plain = twin.collect(T_, out="fresh", policies=kc["policies"], search=dict(kc["search"], noise=0))
        out = ref.collect(T_, out="fresh", **kc)
        for k in KEYS:
            assert torch.equal(out[k], seen[i][k].cpu()), (i, k)
    assert torch.equal(env.squares.cpu(), ref.squares) and torch.equal(env.turn.cpu(), ref.turn)
    assert not torch.equal(seen[0]["actions"], seen[1]["actions"]) and not torch.equal(plain["visits"], seen[0]["visits"].cpu())
