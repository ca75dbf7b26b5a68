"""gbl_train_step_weighted and gbl_replay_importance on the MI355X (-m gpu): the kernels against the host flavour bit for bit (which
tests/test_train_weighted.py holds to the numpy restatement of the header) -- every output and the workspace behind guard bytes, one
step and twenty consecutive ones, on a stream of its own, twice from the same state, every hidden size (each its own instantiation)
--, weights of 1 against gbl_train_step on the device, and the whole loss-driven fit loop against the host flavour."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_restatement as R
from tests import train_weighted_restatement as W
from tests.test_gpu_symmetry import DEV, Guarded, dev
from tests.test_gpu_train_step import device_step, guarded
from tests.test_train_weighted import PRIO, PRIORITY, priorities
from tests.search_harness import G  # noqa: F401  (G: the fixture)

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(b, h) for b in (1, 3, 65, 130) for h in (64, 256)] + [(65, 128), (65, 192)]


def device_weighted(lib, obs, mask, visits, z, hidden, params, m, v, hy, weights=None, prio=None, stream=None):
    """gbl_train_step_weighted on device copies: W.run_step's tuple, every output and the workspace read back through guards."""
    B, P = len(obs), R.param_count(hidden)
    ins = [dev(np.ascontiguousarray(obs, np.int8)), None if mask is None else dev(np.ascontiguousarray(mask, np.int8)),
           dev(np.ascontiguousarray(visits, np.int16)), dev(np.ascontiguousarray(z, np.int8)),
           None if weights is None else dev(np.ascontiguousarray(weights, F))]
    pg, mg, vg = (guarded(np.asarray(a, F)) for a in (params, m, v))
    gg, sg, rl = Guarded((P,), F), Guarded((4,), F), Guarded((B, 2), F)
    po = None if prio is None else Guarded((B,), np.int32)
    scale, floor, cap = (0.0, 0, 0) if prio is None else prio
    ws = Guarded((lib.gbl_train_workspace_bytes(B, hidden),), np.uint8)
    hs = R.hyper_struct(hy)
    s = torch.cuda.current_stream(DEV) if stream is None else stream
    torch.cuda.synchronize()                        # (the copies above ran on the default stream)
    rc = lib.gbl_train_step_weighted(ins[0].data_ptr(), None if ins[1] is None else ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(),
                                     B, hidden, pg.ptr, mg.ptr, vg.ptr, C.addressof(hs), None if ins[4] is None else ins[4].data_ptr(),
                                     rl.ptr, None if po is None else po.ptr, float(scale), int(floor), int(cap), gg.ptr, sg.ptr, ws.ptr,
                                     ws.nbytes, s.cuda_stream)
    assert rc == 0, lib.gbl_last_error()
    s.synchronize()
    ws.read()                                       # (the workspace's guards)
    return (pg.read().copy(), mg.read().copy(), vg.read().copy(), gg.read().copy(), sg.read().copy(), rl.read().copy(),
            None if po is None else po.read().copy())


@pytest.mark.parametrize("B,H", SHAPES)
def test_device_equals_host_flavour(G, B, H):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    side = torch.cuda.Stream(DEV)
    for with_mask in (True, False):
        p = R.init_params(H, H)
        m, v = np.zeros_like(p), np.zeros_like(p)
        for t in range(1, 21):                      # one step, and twenty consecutive ones, a fresh batch and fresh weights each
            obs, mask, visits, z = R.random_batch(B, 5 * B + H + t, with_mask)
            w, hy = W.random_weights(B, B + t), R.hyper_at(t)
            exp = W.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, w, PRIO)
            got = device_weighted(lib, obs, mask, visits, z, H, p, m, v, hy, w, PRIO, stream=side if t % 2 else None)
            W.same_bits(got, exp, (B, H, with_mask, t))
            if t in (1, 20):                        # the same state again: the same bits
                torch.cuda.current_stream(DEV).synchronize()
                W.same_bits(device_weighted(lib, obs, mask, visits, z, H, p, m, v, hy, w, PRIO), got, "second run")
            p, m, v = got[:3]
        assert np.isfinite(p).all() and got[4][2] == (B if B < 4 else B - 2)


@pytest.mark.parametrize("B,H", [(130, 64), (65, 128), (65, 192), (130, 256)])
def test_weights_of_one_equal_gbl_train_step_on_the_device(G, B, H):
    lib = G._native.lib()
    obs, mask, visits, z = R.random_batch(B, 3 * B + H)
    p = R.init_params(H, H)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in (1, 2):
        hy = R.hyper_at(t)
        plain = device_step(lib, obs, mask, visits, z, H, p, m, v, hy)
        W.same_bits(device_weighted(lib, obs, mask, visits, z, H, p, m, v, hy, np.ones(B, F), PRIO), plain, (B, H, t, "ones"))
        W.same_bits(device_weighted(lib, obs, mask, visits, z, H, p, m, v, hy, None, None), plain, (B, H, t, "NULL"))
        p, m, v = plain[:3]


@pytest.mark.parametrize("edge", ["none counted", "open rows", "one candidate"])
def test_edge_batches_equal_host_flavour(G, edge):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    obs, mask, visits, z, H, p, _ = R.EDGES[edge]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    w = W.random_weights(len(obs), 11, special=False)
    for prio in (PRIO, (0.0, 3, 9), (1e30, 2, 77)):
        W.same_bits(device_weighted(lib, obs, mask, visits, z, H, p, m, v, hy, w, prio),
                    W.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, w, prio), (edge, prio))


def test_several_rounds_of_the_grid_stride_loop(G):
    """2 100 rows at H = 256 are more than the weighted row kernel's 512 workgroups of four wavefronts hold at once."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    obs, mask, visits, z = R.random_batch(2100, 256)
    p = R.init_params(256, 3)
    m, v, hy, w = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1), W.random_weights(2100, 5)
    W.same_bits(device_weighted(lib, obs, mask, visits, z, 256, p, m, v, hy, w, PRIO), W.run_step(cpu, obs, mask, visits, z, 256, p, m, v, hy, w, PRIO))


@pytest.mark.parametrize("n", [1, 64, 65, 4097, 65536])
def test_importance_equals_host_flavour(G, n):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    side = torch.cuda.Stream(DEV)
    for seed, beta in enumerate((0.0, 0.4, 1.0)):
        p = priorities(n, 100 * n + seed)
        dead = -np.abs(p)                            # the all-failed batch: no entry positive
        dead[::3] = 0
        for prio, stream in ((p, side), (dead, torch.cuda.current_stream(DEV))):
            d, out = dev(prio), Guarded((n,), F)
            torch.cuda.synchronize()
            assert lib.gbl_replay_importance(d.data_ptr(), n, beta, out.ptr, stream.cuda_stream) == 0, lib.gbl_last_error()
            stream.synchronize()
            got = out.read()
            assert np.array_equal(got.view(np.uint32), W.run_importance(cpu, prio, beta).view(np.uint32)), (n, beta)
        assert not got.any()


def test_the_loss_driven_fit_equals_the_host_flavour(G):
    """The 8-step fit(..., beta, priority) on a 64-board x 8-ply ring, on one stream with no synchronisation in between: params, the
    moments and the ring's priorities agree with the host flavour byte for byte."""
    search = dict(iterations=8, playouts=2, sample_plies=4)
    bufs, trainers, stats = {}, {}, {}
    for d in (DEV, "cpu"):
        env = G.BatchedGobblet(64, d, auto_reset=True, seed=5, track_turn=True)
        traj = env.collect(8, policies=("tree", "tree"), search=search)
        env.outcome_targets(traj)
        bufs[d] = G.ReplayBuffer(1024, d, prioritized=True)
        bufs[d].append(env, traj, tag=1, priority=7)
        trainers[d] = G.GobbletTrainer(hidden=64, device=d, seed=1)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        stats[DEV] = bufs[DEV].fit(trainers[DEV], 8, batch=64, first_call=3, prioritized=True, beta=0.5, priority=PRIORITY)
    torch.cuda.synchronize()
    stats["cpu"] = bufs["cpu"].fit(trainers["cpu"], 8, batch=64, first_call=3, prioritized=True, beta=0.5, priority=PRIORITY)
    assert torch.equal(stats[DEV].cpu(), stats["cpu"]) and float(stats["cpu"][:, 2].min()) == 64
    for name in ("params", "m", "v", "last_grad", "hidden_max", "last_row_loss", "last_priority"):
        assert getattr(trainers[DEV], name).cpu().numpy().tobytes() == getattr(trainers["cpu"], name).numpy().tobytes(), name
    assert bufs[DEV].priority.cpu().numpy().tobytes() == bufs["cpu"].priority.numpy().tobytes()
    assert (bufs["cpu"].priority[:bufs["cpu"].size] != 7).any()
