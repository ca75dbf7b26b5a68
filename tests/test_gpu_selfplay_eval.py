"""gbl_collect_search_eval on the MI355X (-m gpu): k_collect_eval against the host flavour and against the Python restatement of the
contract, bit for bit and with canaries around every output; against the composed loop of gbl_tree_search_eval + gbl_step_into on
the device; a batch beyond the grid cap; a graph capture with the weights refreshed in place; NULL optional outputs; and
BatchedGobblet.collect with two policy instances.  (k_collect_eval has one instantiation -- one wavefront per board -- so the
batch sizes are those of cell()'s tile edge: 1, 3, 63, 64, 65 and 257 boards.)"""
import os
import sys

import numpy as np
import pytest
import torch

from tests import evaluator_restatement as R
from tests import selfplay_harness as H
from tests.search_harness import G, midgame_boards  # noqa: F401  (G: the fixture)
from tests.selfplay_harness import DEV, DeviceNet, same
from tests.test_selfplay_eval import collect_eval, restate_collect

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
GRID_CAP = 1 << 20


@pytest.fixture(scope="module")
def c5(G):
    return midgame_boards(turn=True)


def host_collect(G, *args, **kw):
    cpu = G._native.cpu_raw()
    return collect_eval(cpu.gbl_cpu_collect_search_eval, cpu.gbl_cpu_last_error, *args, **kw)


# gbl_collect_search_eval on the device, every output between canaries (H.device_collect), under collect_eval's argument order
device_collect = lambda G, st, tm, turn, T, pols, dnets, its, X, *a, **kw: H.device_collect("eval", st, tm, turn, T, pols, X, *a, nets=dnets, its=its, **kw)  # noqa: E731


def pair(h0, h1):
    nets = (R.random_net(h0, 5 + h0), R.random_net(h1, 9 + h1))
    return nets, tuple(DeviceNet(x) for x in nets)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257])
def test_device_equals_host_flavour(G, c5, n):
    st, tm, turn = c5[0][:n], c5[1][:n], c5[2][:n] % 5
    for (h0, h1), its, T, layout, sp, mode in (((64, 256), (64, 2), 5, "time", 2, 0), ((128, 192), (1, 64), 5, "tile", 0, 1),
                                               ((256, 64), (2, 1), 1, "time", 2, 1), ((192, 128), (2, 2), 1, "tile", 0, 0)):
        nets, dnets = pair(h0, h1)
        args = (its, 48, sp, mode, layout, 3, 17, 4)
        same(device_collect(G, st, tm, turn, T, ("eval", "eval"), dnets, *args), host_collect(G, st, tm, turn, T, ("eval", "eval"), nets, *args))
    nets, dnets = pair(64, 128)  # a random side, NULL for its evaluator, the ply index through ply_dev
    args = ((0, 64), 16, 2, 0, "time", 1, 0, 0, 7)
    same(device_collect(G, st, tm, turn, 5, ("random", "eval"), (None, dnets[1]), *args),
         host_collect(G, st, tm, turn, 5, ("random", "eval"), (None, nets[1]), *args))


def test_device_equals_host_flavour_at_512_iterations(G, c5):
    """The LDS limit (36.9 KB of tree) and the widest prior-row offset: 3 boards, 2 plies."""
    nets, dnets = pair(256, 64)
    args = (2, ("eval", "eval"), None, (512, 512), 64, 0, 0, "time", 1, 0, 0)
    st, tm, turn = c5[0][:3], c5[1][:3], c5[2][:3]
    got = device_collect(G, st, tm, turn, *args[:2], dnets, *args[3:])
    same(got, host_collect(G, st, tm, turn, *args[:2], nets, *args[3:]))
    assert (got[0]["visits"].sum(2) == 512).all() and (got[0]["nodes"] <= 513).all()


@pytest.mark.parametrize("pols,its,sample_plies,illegal_mode", [(("eval", "eval"), (8, 3), 2, 0), (("eval", "random"), (1, 1), 0, 1),
                                                                  (("random", "eval"), (2, 64), 2, 1)])
def test_device_equals_restatement(G, c5, pols, its, sample_plies, illegal_mode):
    st = np.concatenate([np.zeros((2, 27), np.int8), c5[0][:4]])
    tm = np.concatenate([np.zeros(2, np.int8), c5[1][:4]])
    turn = np.concatenate([np.zeros(2, np.int32), c5[2][:4] % 4])  # (some of them inside the sampled plies)
    nets, dnets = pair(64, 256)
    seed, env_base, ply0, T = 9, (1 << 40) - 20, 5, 5
    exp = restate_collect(st, tm, turn, T, pols, nets, its, 48, sample_plies, illegal_mode, seed, env_base, ply0 + 3)
    for layout in ("time", "tile"):
        same(device_collect(G, st, tm, turn, T, pols, dnets, its, 48, sample_plies, illegal_mode, layout, seed, env_base, ply0, 3), exp)


def test_device_equals_composed_loop(G, c5):
    import bench_selfplay_eval as B
    r = B.Runner(torch.from_numpy(c5[0][:256]).to(DEV), torch.from_numpy(c5[1][:256]).to(DEV), 32, B.seeded_evaluator(128), plies=8, seed=5)
    r.check_equal()


def test_null_optional_outputs(G, c5):
    nets, dnets = pair(128, 64)
    st, tm, turn = c5[0][:130], c5[1][:130], c5[2][:130] % 3
    args = (3, ("eval", "eval"), dnets, (24, 12), 64, 2, 0, "time", 3, 0, 0)
    full = device_collect(G, st, tm, turn, *args)
    for keep in (("actions",), ("visits", "root_value"), ("priors",), ("value", "nodes", "how", "mover", "observation"), ("action_mask", "priors"), ()):
        got = device_collect(G, st, tm, turn, *args, keep=keep)
        assert set(got[0]) == set(keep)
        same(got, full)


def test_beyond_the_grid_cap(G, c5):
    """2^20 + 65 boards: the grid-stride loop's second trip runs on 65 workgroups, and must keep nothing of the first trip's tree or
    turn counter."""
    n = GRID_CAP + 65
    st, tm, turn = np.resize(c5[0], (n, 27)), np.resize(c5[1], n), np.resize(c5[2] % 3, n)
    nets, dnets = pair(64, 64)
    keep = ("actions", "visits", "nodes", "root_value")
    # (env_base 0 and sample_plies 0: a searching board's plies depend on the board alone, so the batch repeats its head)
    args = (2, ("eval", "eval"), None, (1, 1), 64, 0, 0, "tile", 3, 0, 0)
    got = device_collect(G, st, tm, turn, *args[:2], dnets, *args[3:], keep=keep)
    head = host_collect(G, st[:65536], tm[:65536], turn[:65536], *args[:2], nets, *args[3:], keep=keep)
    for k in keep:
        assert np.array_equal(got[0][k], head[0][k][:, np.arange(n) % 65536]), k
    assert np.array_equal(got[1], np.resize(head[1], (n, 27))) and np.array_equal(got[4], np.resize(head[4], n))


def test_graph_capture_with_weights_refreshed_in_place(G, c5):
    """One captured launch with ply_dev, replayed three times; gbl_counter_add advances the ply inside the graph and the weights are
    overwritten in place between the replays: the same as three eager launches with the three weight sets."""
    nat = G._native
    n, T, seed = 300, 3, 7
    sets = [R.random_net(64, 30 + i) for i in range(3)]
    ev = G.GobbletEvaluator(sets[0].w1, sets[0].b1, sets[0].w2, sets[0].b2, 1, 9, 9, device=DEV)
    pol = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=16)
    kw = dict(policies=(pol, "random"), search=dict(sample_plies=2))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    env.rollout(3)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T, search_outputs=True, evaluator_outputs=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    seen = []
    keys = ("actions", "visits", "value", "how", "mover", "root_value", "priors", "observation")
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            env.collect(T, out=buf, **kw)
            env.advance_ply()
        for i in range(3):
            for dst, src in zip((ev.w1, ev.b1, ev.w2, ev.b2), (sets[i].w1, sets[i].b1, sets[i].w2, sets[i].b2)):
                dst.copy_(torch.from_numpy(src))  # in place: the captured launch holds these addresses
            g.replay()
            side.synchronize()
            seen.append({k: buf[k].clone() for k in keys})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    ref.load_state_dict(sd)
    for i in range(3):
        e = G.GobbletEvaluator(sets[i].w1, sets[i].b1, sets[i].w2, sets[i].b2, 1, 9, 9, device=DEV)
        out = ref.collect(T, out="fresh", policies=(G.EvaluatorTreeSearchGobbletPolicy(e, iterations=16), "random"), search=dict(sample_plies=2))
        for k in keys:
            assert torch.equal(out[k], seen[i][k]), (i, k)
    assert torch.equal(env.squares, ref.squares) and torch.equal(env.turn, ref.turn)
    assert not torch.equal(seen[0]["visits"], seen[1]["visits"])
    assert nat.POLICY_EVAL_TREE == 5


def test_collect_with_two_policy_instances(G, c5):
    nets = (R.random_net(64, 3), R.random_net(192, 4))
    evs = [G.GobbletEvaluator(x.w1, x.b1, x.w2, x.b2, x.shift1, x.shift_p, x.shift_v, device=DEV) for x in nets]
    pols = [G.EvaluatorTreeSearchGobbletPolicy(e, iterations=i, explore=24) for e, i in zip(evs, (20, 9))]
    env = G.BatchedGobblet(200, DEV, auto_reset=True, seed=4, env_base=3, track_turn=True)
    env.rollout(5)
    torch.cuda.synchronize()
    st, tm, turn, ply = env.squares.cpu().numpy().copy(), env.to_move.cpu().numpy().copy(), env.turn.cpu().numpy().copy(), env.ply
    out = env.collect(4, policies=pols, search=dict(sample_plies=6), count=True)
    env.outcome_targets(out)
    torch.cuda.synchronize()
    exp = host_collect(G, st, tm, turn, 4, ("eval", "eval"), nets, (20, 9), 24, 6, 0, "time", 4, 3, ply)
    for k in exp[0]:
        assert np.array_equal(out[k].cpu().numpy().reshape(exp[0][k].shape), exp[0][k]), k
    assert np.array_equal(env.squares.cpu().numpy(), exp[1]) and int(env.counters[0]) == 200 * 4 and out["z"].dtype == torch.int8
    with pytest.raises(ValueError, match="lives on"):
        env.collect(2, policies=("evaluator", "random"), search=dict(evaluator=evs[0].to("cpu")))
