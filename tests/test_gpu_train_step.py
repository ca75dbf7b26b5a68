"""gbl_train_step on the MI355X (-m gpu): the two kernels against the host flavour bit for bit (which tests/test_train_step.py holds to
the numpy restatement of the header) -- every output and the workspace behind guard bytes, one step and twenty consecutive ones, on
a stream of its own, twice from the same state -- on the host tests' shapes and edge batches, and BatchedGobblet.fit against the
hand-written loop and the host flavour."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import train_restatement as R
from tests.test_gpu_symmetry import DEV, GUARD, Guarded, dev
from tests.test_train_step import SHAPES
from tests.search_harness import G  # noqa: F401  (G: the fixture)

pytestmark = pytest.mark.gpu

F = np.float32


def guarded(a):
    """A guarded device copy of the numpy array a."""
    g = Guarded(a.shape, a.dtype)
    g.raw[GUARD:GUARD + g.nbytes] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)
    return g


def device_step(lib, obs, mask, visits, z, hidden, params, m, v, hy, stream=None, grad=True):
    """gbl_train_step on device copies: (params', m', v', g or None, stats), every output and the workspace read back through guards."""
    B, P = len(obs), R.param_count(hidden)
    ins = [dev(np.ascontiguousarray(obs, np.int8)), None if mask is None else dev(np.ascontiguousarray(mask, np.int8)),
           dev(np.ascontiguousarray(visits, np.int16)), dev(np.ascontiguousarray(z, np.int8))]
    pg, mg, vg = (guarded(np.asarray(a, F)) for a in (params, m, v))
    gg, sg = (Guarded((P,), F) if grad else None), Guarded((4,), F)
    ws = Guarded((lib.gbl_train_workspace_bytes(B, hidden),), np.uint8)
    hs = R.hyper_struct(hy)
    s = torch.cuda.current_stream(DEV) if stream is None else stream
    torch.cuda.synchronize()                        # (the copies above ran on the default stream)
    rc = lib.gbl_train_step(ins[0].data_ptr(), None if ins[1] is None else ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), B,
                            hidden, pg.ptr, mg.ptr, vg.ptr, C.addressof(hs), None if gg is None else gg.ptr, sg.ptr, ws.ptr, ws.nbytes,
                            s.cuda_stream)
    assert rc == 0, lib.gbl_last_error()
    s.synchronize()
    ws.read()                                       # (the workspace's guards)
    return pg.read().copy(), mg.read().copy(), vg.read().copy(), None if gg is None else gg.read().copy(), sg.read().copy()


@pytest.mark.parametrize("B,H", SHAPES)
def test_device_equals_host_flavour(G, B, H):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    side = torch.cuda.Stream(DEV)
    for with_mask in (True, False):
        p = R.init_params(H, H)
        m, v = np.zeros_like(p), np.zeros_like(p)
        for t in range(1, 21):                      # one step, and twenty consecutive ones, a fresh batch each
            obs, mask, visits, z = R.random_batch(B, 7 * B + H + t, with_mask)
            hy = R.hyper_at(t)
            exp = R.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy)
            got = device_step(lib, obs, mask, visits, z, H, p, m, v, hy, stream=side if t % 2 else None)
            R.same_bits(got, exp, (B, H, with_mask, t))
            if t in (1, 20):                        # the same state again: the same bits; and grad_out is optional
                torch.cuda.current_stream(DEV).synchronize()
                R.same_bits(device_step(lib, obs, mask, visits, z, H, p, m, v, hy, grad=t == 1), got, "second run")
            p, m, v = got[:3]
        assert np.isfinite(p).all() and got[4][2] == (B if B < 4 else B - 2)


@pytest.mark.parametrize("edge", sorted(R.EDGES))
def test_edge_batches_equal_host_flavour(G, edge):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    obs, mask, visits, z, H, p, off = R.EDGES[edge]()
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in (1, 2):
        hy = R.hyper_at(t, **off)
        exp = R.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy)
        got = device_step(lib, obs, mask, visits, z, H, p, m, v, hy)
        R.same_bits(got, exp, (edge, t))
        p, m, v = got[:3]
    assert all(np.isfinite(a).all() for a in got)


@pytest.mark.parametrize("B,H", [(1100, 128), (1100, 192), (2100, 256)])
def test_the_other_hidden_sizes_and_several_rounds(G, B, H):
    """1 100 rows are 18 chunks, so the reduction's 16 wavefronts go round twice; 2 100 rows at H = 256 are more than the row kernel's
    512 workgroups of four wavefronts hold at once, so its wavefronts take a second row (the grid-stride loop)."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    obs, mask, visits, z = R.random_batch(B, H)
    p = R.init_params(H, 3)
    m, v = np.zeros_like(p), np.zeros_like(p)
    hy = R.hyper_at(1)
    R.same_bits(device_step(lib, obs, mask, visits, z, H, p, m, v, hy), R.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy), (B, H))


def test_fit_equals_the_loop_and_the_host_flavour(G):
    """10 steps on a 64-board x 8-ply window: BatchedGobblet.fit, the hand-written loop of training_batch + step, the host flavour."""
    search = dict(iterations=8, playouts=2, sample_plies=4)
    envs, trajs = {}, {}
    for d in (DEV, "cpu"):
        envs[d] = G.BatchedGobblet(64, d, auto_reset=True, seed=23, track_turn=True)
        trajs[d] = envs[d].collect(8, policies=("tree", "tree"), search=search)
        envs[d].outcome_targets(trajs[d])
    assert torch.equal(trajs[DEV]["visits"].cpu(), trajs["cpu"]["visits"]) and torch.equal(trajs[DEV]["z"].cpu(), trajs["cpu"]["z"])
    fitted, looped, host = (G.GobbletTrainer(hidden=64, device=d, seed=4) for d in (DEV, DEV, "cpu"))
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        stats = envs[DEV].fit(trajs[DEV], fitted, 10, batch=256, first_call=3)
    torch.cuda.synchronize()
    by_hand = []
    for i in range(10):
        by_hand.append(looped.step(envs[DEV].training_batch(trajs[DEV], 256, symmetries="all", call=3 + i)))
    host_stats = envs["cpu"].fit(trajs["cpu"], host, 10, batch=256, first_call=3)
    assert stats.shape == (10, 4) and float(stats[:, 2].min()) > 0 and fitted.t == looped.t == host.t == 10
    assert torch.equal(stats, torch.stack(by_hand)) and torch.equal(stats.cpu(), host_stats)
    for name in ("params", "m", "v", "last_grad", "hidden_max"):
        assert torch.equal(getattr(fitted, name), getattr(looped, name)), name
        assert torch.equal(getattr(fitted, name).cpu(), getattr(host, name)), name
    ev, ev_host = fitted.evaluator(), host.evaluator()
    assert torch.equal(ev.w1.cpu(), ev_host.w1) and torch.equal(ev.w2.cpu(), ev_host.w2) and ev.shift1 == ev_host.shift1
