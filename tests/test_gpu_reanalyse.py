"""k_reanalyse on the MI355X (-m gpu) against the host flavour byte for byte (which tests/test_reanalyse.py holds to the restatement of
the header's rule), every array read back through guard bytes and padding: the CPU test's rows at 1, 8, 64 and 512 iterations (the
largest tree the LDS holds), H = 64 and 256, a batch's pitches and the ring's, in place and not; one row, the rows around a
wavefront's 64, and one more row than the capped grid has workgroups (2^20 + 1); the kernel against gbl_decode_obs +
gbl_tree_search_eval on the device; the fixed point and the untouched ring bytes; and a fit with reanalyse= against the same fit on the
host flavour."""
import ctypes as C

import numpy as np
import pytest
import torch

from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as ER
from tests import reanalyse_harness as H
from tests.search_harness import G  # noqa: F401  (the fixture)
from tests.tb_targets_harness import BATCH, RING

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAP = 1 << 20   # knob::kReanalyseGroups: the workgroups of the largest grid, one row each per pass
EXPLORE = H.EXPLORE


@pytest.fixture(scope="module")
def rows(G):
    return H.make_rows(H.net64())


def same(dev, host, what, *args, **kw):
    got, exp = H.run(dev, *args, **kw), H.run(host, *args, **kw)
    assert set(got) == set(exp)
    for k in exp:
        assert got[k].tobytes() == exp[k].tobytes(), (what, k, np.argwhere(got[k] != exp[k])[:5])
    return exp


@pytest.mark.parametrize("hidden", [64, 256])
@pytest.mark.parametrize("iterations", [1, 8, 64, 512])
def test_kernel_equals_the_host_flavour(rows, hidden, iterations):
    net = H.net64() if hidden == 64 else ER.random_net(256, 261)
    dev, host = H.Env(net, DEV), H.Env(net, "cpu")
    obs, mask, v_old, z_old = rows
    pick = np.arange(257) * 7 % len(obs)
    obs, mask, v_old, z_old = obs[pick], mask[pick], v_old[pick], z_old[pick]
    for layout, inplace, lead in ((BATCH, True, 0), (RING, True, 1), (RING, False, 0), (BATCH, False, 1)):
        exp = same(dev, host, (layout is RING, inplace, lead), obs, mask, v_old, z_old, iterations, layout=layout, inplace=inplace, lead=lead)
    live = exp["census"] >= 0
    assert live.sum() > 60 and (exp["visits"][live].sum(1) == iterations).all() and (z_old == nat.Z_OPEN).any()
    same(dev, host, "no optional input", obs, None, None, None, iterations, keep=("drift", "census", "nodes"))
    same(dev, host, "the empty mask", obs, np.zeros_like(mask), v_old, z_old, iterations)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_row_counts_around_a_wavefront(rows, n):
    dev, host = H.Env(H.net64(), DEV), H.Env(H.net64(), "cpu")
    obs, mask, v_old, z_old = (a[:n] for a in rows)
    for layout in (BATCH, RING):
        same(dev, host, n, obs, mask, v_old, z_old, 8, layout=layout)


def test_a_second_trip_through_the_grid_stride_loop(rows):
    """One more row than the grid has workgroups, at one iteration, the ring's pitches in place: workgroup 0 takes row 0 and the last
    row.  The rows repeat the module's rows, so row r must come out as row r % P of a small launch (which the tests above hold to the
    host flavour); the arrays are built and compared with torch on the device, junk in the padding."""
    net = H.net64()
    dev = H.Env(net, DEV)
    base = [np.concatenate([a[:180], a[-20:]]) for a in rows]          # (self-play rows and masked-random ones, skipped rows among them)
    assert (base[3] == nat.Z_OPEN).any()
    P, n = 200, GRID_CAP + 1
    small = H.run(dev, *base, 1, layout=RING, keep=("drift", "census", "action"))
    pick = torch.arange(n, device=DEV) % P
    pick[-1] = 5                                                       # (not the row workgroup 0 began with)
    obs, mask, v_old, z_old = (torch.from_numpy(a).to(DEV)[pick] for a in base)
    ring_obs = torch.full((n, 128), 0x5A, dtype=torch.int8, device=DEV)
    ring_meta = torch.full((n, 64), 0x5A, dtype=torch.int8, device=DEV)
    ring_visits = torch.full((n, 64), 0x5A5A, dtype=torch.int16, device=DEV)
    ring_obs[:, :117], ring_meta[:, :54], ring_meta[:, 54], ring_visits[:, :54] = obs, mask, z_old, v_old
    obs_was, meta_was = ring_obs.clone(), ring_meta.clone()
    out = {k: torch.full((n,), -99, dtype=dt, device=DEV) for k, dt in (("action", torch.int32), ("drift", torch.int32), ("census", torch.int8))}
    ev = net.struct(dev.arrays)
    rc = dev.L.gbl_reanalyse(C.addressof(ev), 1, EXPLORE, ring_obs.data_ptr(), 128, ring_meta.data_ptr(), 64, ring_visits.data_ptr(),
                             ring_visits.data_ptr(), 64, ring_meta.data_ptr() + 54, 64, None, None, out["action"].data_ptr(), None,
                             out["drift"].data_ptr(), out["census"].data_ptr(), n, dev.stream)
    assert rc == 0, dev.error()
    torch.cuda.synchronize()
    assert torch.equal(ring_obs, obs_was) and torch.equal(ring_meta, meta_was) and (ring_visits[:, 54:] == 0x5A5A).all()
    assert torch.equal(ring_visits[:, :54], torch.from_numpy(small["visits"]).to(DEV)[pick])
    for k in out:
        assert torch.equal(out[k], torch.from_numpy(small[k]).to(DEV)[pick]), k
    assert int(out["action"][-1]) == int(small["action"][5]) >= 0


def test_kernel_equals_decode_and_search_on_the_device(rows):
    net = H.net64()
    dev = H.Env(net, DEV)
    obs, mask, v_old, z_old = rows
    n = len(obs)
    got = H.run(dev, obs, mask, v_old, None, 64, inplace=False)        # (no z: no row is skipped)
    d_obs, d_mask = torch.from_numpy(obs).to(DEV), torch.from_numpy(mask).to(DEV)
    state, who = torch.empty((n, 27), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)
    out = {k: torch.empty((n, 54) if k in ("visits", "wins", "losses") else n, dtype=torch.int32, device=DEV)
           for k in ("visits", "wins", "losses", "action", "nodes", "root_value")}
    priors = torch.empty((n, 54), dtype=torch.uint8, device=DEV)
    ev = net.struct(dev.arrays)
    assert dev.L.gbl_decode_obs(d_obs.data_ptr(), state.data_ptr(), who.data_ptr(), n, dev.stream) == 0
    assert dev.L.gbl_tree_search_eval(state.data_ptr(), who.data_ptr(), d_mask.data_ptr(), C.addressof(ev), 64, EXPLORE, *[out[k].data_ptr() for k in out],
                                      priors.data_ptr(), n, dev.stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(got["visits"], out["visits"].cpu().numpy().astype(np.int16))
    for k in ("action", "nodes", "root_value"):
        assert np.array_equal(got[k], out[k].cpu().numpy()), k
    assert np.array_equal(got["root_priors"], priors.cpu().numpy())


def test_fixed_point_doubling_and_untouched_ring_bytes_on_the_device(G):
    from tests.test_reanalyse import check_fixed_point_and_untouched_bytes
    buf, ev, out = check_fixed_point_and_untouched_bytes(DEV)
    cbuf, cev, cout = check_fixed_point_and_untouched_bytes("cpu")
    assert torch.equal(buf._visits.cpu(), cbuf._visits) and torch.equal(out["drift"].cpu(), cout["drift"])


def test_fit_with_reanalyse_equals_the_host_flavour(G):
    fits = []
    for d in (DEV, "cpu"):
        buf, ev = H.selfplay_ring(H.net64(), d, iterations=8, sample_plies=4, capacity=600, prioritized=True)
        trainer = G.GobbletTrainer(hidden=64, device=d, seed=1)
        spec = dict(evaluator=ev, iterations=16, explore=EXPLORE)
        stats = [buf.fit(trainer, 2, batch=128, first_call=5, reanalyse=spec),
                 buf.fit(trainer, 2, batch=128, first_call=9, reanalyse=spec, prioritized=True, beta=0.5, priority=dict(scale=64.0, floor=1, cap=1 << 20))]
        fits.append((torch.cat(stats).cpu(), trainer.params.cpu(), trainer.m.cpu(), trainer.v.cpu(), buf.priority.cpu()))
    for a, b in zip(*fits):
        assert torch.equal(a, b)
    assert float(fits[1][0][:, 2].min()) > 0
