"""k_reanalyse<true> on the MI355X (-m gpu) against the host flavour byte for byte (which tests/test_reanalyse_gumbel.py holds to the
restatement of the header's rule), every array read back through guard bytes and padding: 1 / 65 / 130 rows (one row, one past a
wavefront's worth of workgroups, a ragged tail) with skipped rows and rows without a candidate interleaved, the (considered, iterations)
pairs of the CPU test with noise and scale off and on, H = 64 and 128, a batch's pitches and the ring's in place; the alignment rules;
the drift's largest operands; the identity on a Gumbel ring; a fit with reanalyse=dict(gumbel=...) against the host flavour; and
gbl_reanalyse, still byte-equal to the host flavour."""
import numpy as np
import pytest
import torch

from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as ER
from tests import reanalyse_gumbel_harness as GH
from tests import reanalyse_harness as H
from tests.search_harness import G  # noqa: F401  (the fixture)
from tests.tb_targets_harness import BATCH, RING

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXPLORE = GH.EXPLORE
SEED, ENV_BASE, CALL = 0x123456789ABCDEF, (1 << 33) + 5, 77
PAIRS = [(1, 8), (3, 8), (16, 16), (16, 64), (54, 16)]                 # (considered, iterations)


@pytest.fixture(scope="module")
def rows(G):
    """130 rows: the planted rows (every kind: 54 / 27 / 3 / 2 / 1 / 0 candidates, skipped rows, the old rows' edges) between
    masked-random ones, every fifth of those skipped or without a candidate in turn."""
    obs, mask, v_old, z_old = GH.planted_rows()
    r_obs, r_mask = H.random_rows(110, 31)
    rng = np.random.default_rng(32)
    r_mask = r_mask.copy()
    r_v = (rng.integers(0, 256, (110, 54)) * (rng.random((110, 54)) < 0.5)).astype(np.int16) * (r_mask != 0)
    r_z = rng.choice(np.array([-1, 0, 1], np.int8), 110)
    r_z[0::10] = nat.Z_OPEN
    r_mask[5::10] = 0
    order = rng.permutation(130)
    return tuple(np.concatenate(p)[order] for p in ((obs, r_obs), (mask, r_mask), (v_old, r_v), (z_old, r_z)))


def same(dev, host, what, *args, **kw):
    got, exp = GH.run(dev, *args, **kw), GH.run(host, *args, **kw)
    assert set(got) == set(exp)
    for k in exp:
        assert got[k].tobytes() == exp[k].tobytes(), (what, k, np.argwhere(got[k] != exp[k])[:5])
    return exp


@pytest.mark.parametrize("noise,scale", [(0, 0), (1, 23)])
@pytest.mark.parametrize("considered,iterations", PAIRS)
@pytest.mark.parametrize("hidden", [64, 128])
def test_kernel_equals_the_host_flavour(rows, hidden, considered, iterations, noise, scale):
    net = H.net64() if hidden == 64 else ER.random_net(128, 133)
    dev, host = H.Env(net, DEV), H.Env(net, "cpu")
    rule = (considered, noise, 50, scale)
    for n, layout, inplace, lead in ((130, RING, True, 0), (65, BATCH, False, 1), (1, RING, True, 1), (130, BATCH, True, 3)):
        obs, mask, v_old, z_old = (a[:n] for a in rows)
        exp = same(dev, host, (n, layout is RING, inplace), obs, mask, v_old, z_old, iterations, rule, SEED, ENV_BASE, CALL, layout=layout,
                   inplace=inplace, lead=lead)
    live = exp["census"] >= 0
    assert live.sum() > 90 and (rows[3] == nat.Z_OPEN).sum() > 10 and ((exp["action"] == -1) & (exp["nodes"] == 1)).sum() > 10
    assert (exp["visits"][live].max(1) <= 255).all() and (exp["gumbel"] != 0).any() == bool(noise)


def test_optional_inputs_and_outputs(rows):
    dev, host = H.Env(H.net64(), DEV), H.Env(H.net64(), "cpu")
    obs, mask, v_old, z_old = rows
    same(dev, host, "no optional input", obs, None, None, None, 16, GH.RULE, SEED, ENV_BASE, CALL, keep=("drift", "census", "nodes", "gumbel"))
    same(dev, host, "the empty mask", obs, np.zeros_like(mask), v_old, z_old, 16, GH.RULE, SEED, ENV_BASE, CALL)
    same(dev, host, "no visits_out", obs, mask, v_old, z_old, 16, GH.RULE, SEED, ENV_BASE, CALL, inplace=False, give_visits_out=False)
    same(dev, host, "the gumbel row alone", obs, mask, v_old, z_old, 16, GH.RULE, SEED, ENV_BASE, CALL, keep=("gumbel",), layout=RING)


def test_kernel_equals_decode_and_the_gumbel_search_on_the_device(rows):
    import ctypes as C
    net = H.net64()
    dev = H.Env(net, DEV)
    obs, mask, v_old, _ = rows
    n = len(obs)
    got = GH.run(dev, obs, mask, v_old, None, 16, GH.RULE, SEED, ENV_BASE, CALL, inplace=False)          # (no z: no row is skipped)
    d_obs, d_mask = torch.from_numpy(obs).to(DEV), torch.from_numpy(mask).to(DEV)
    state, who = torch.empty((n, 27), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)
    out = {k: torch.empty((n, 54) if k in ("visits", "wins", "losses") else n, dtype=torch.int32, device=DEV)
           for k in ("visits", "wins", "losses", "action", "nodes", "root_value")}
    priors, target = (torch.empty((n, 54), dtype=torch.uint8, device=DEV) for _ in range(2))
    gum = torch.empty((n, 54), dtype=torch.int16, device=DEV)
    ev = net.struct(dev.arrays)
    assert dev.L.gbl_decode_obs(d_obs.data_ptr(), state.data_ptr(), who.data_ptr(), n, dev.stream) == 0
    assert dev.L.gbl_tree_search_gumbel(state.data_ptr(), who.data_ptr(), d_mask.data_ptr(), C.addressof(ev), 16, EXPLORE, *GH.RULE, SEED, ENV_BASE,
                                        CALL, *[out[k].data_ptr() for k in out], priors.data_ptr(), target.data_ptr(), gum.data_ptr(), n,
                                        dev.stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(got["visits"], target.cpu().numpy().astype(np.int16))
    for k in ("action", "nodes", "root_value"):
        assert np.array_equal(got[k], out[k].cpu().numpy()), k
    assert np.array_equal(got["root_priors"], priors.cpu().numpy()) and np.array_equal(got["gumbel"], gum.cpu().numpy())


def test_misaligned_rows_are_refused(G):
    import ctypes as C
    net = H.net64()
    dev = H.Env(net, DEV)
    buf = torch.zeros(1 << 16, dtype=torch.int8, device=DEV)
    base = buf.data_ptr()
    assert base % 64 == 0
    ev = net.struct(dev.arrays)

    def call(**over):
        a = dict(obs=base, visits_in=base + 4096, visits_out=base + 4096, root_value=base + 8192, action=base + 12288, nodes=base + 16384,
                 drift=base + 20480, gumbel=base + 24576)
        a.update(over)
        rc = dev.L.gbl_reanalyse_gumbel(C.addressof(ev), 8, EXPLORE, *GH.RULE, 0, 0, 0, a["obs"], 117, None, 54, a["visits_in"], a["visits_out"], 54, None,
                                        1, a["root_value"], None, a["action"], a["nodes"], a["drift"], None, a["gumbel"], 4, dev.stream)
        return rc, dev.error().decode()
    for over, why in ((dict(visits_in=base + 4097, visits_out=base + 4097), "visits_in must be 2-byte aligned"),
                      (dict(visits_in=None, visits_out=base + 4097), "visits_out must be 2-byte aligned"),
                      (dict(root_value=base + 8194), "4-byte aligned"), (dict(action=base + 12289), "4-byte aligned"),
                      (dict(nodes=base + 16386), "4-byte aligned"), (dict(drift=base + 20483), "4-byte aligned"),
                      (dict(gumbel=base + 24577), "gumbel_out must be 2-byte aligned")):
        rc, msg = call(**over)
        assert rc == nat.ERR_ALIGN and why in msg, (over, rc, msg)
    torch.cuda.synchronize()
    assert not buf.any()                                               # a refused call launches nothing
    assert call()[0] == 0                                              # ... and the aligned one runs (four empty boards)
    torch.cuda.synchronize()
    assert buf[4096:4096 + 4 * 108].any()


def test_drift_edges_on_the_device(G):
    from tests.test_reanalyse_gumbel import check_drift_edges
    got = check_drift_edges(H.Env(ER.zero_net(64), DEV), H.Env(H.net64(), DEV))
    exp = check_drift_edges(H.Env(ER.zero_net(64)), H.Env(H.net64()))
    assert all(got[k].tobytes() == exp[k].tobytes() for k in exp)


def test_identity_on_a_gumbel_ring_on_the_device(G):
    from tests.test_reanalyse_gumbel import check_identity_and_untouched_bytes
    buf, ev, out = check_identity_and_untouched_bytes(DEV)
    cbuf, cev, cout = check_identity_and_untouched_bytes("cpu")
    assert torch.equal(buf._visits.cpu(), cbuf._visits) and torch.equal(out["drift"].cpu(), cout["drift"])


def test_fit_with_gumbel_reanalysis_equals_the_host_flavour(G):
    fits = []
    for d in (DEV, "cpu"):
        buf, ev = GH.gumbel_ring(H.net64(), d, prioritized=True)
        trainer = G.GobbletTrainer(hidden=64, device=d, seed=1)
        spec = dict(evaluator=ev, iterations=16, explore=EXPLORE, gumbel=dict(considered=8), seed=11)
        stats = [buf.fit(trainer, 2, batch=128, first_call=5, reanalyse=spec),
                 buf.fit(trainer, 2, batch=128, first_call=9, reanalyse=spec, prioritized=True, beta=0.5, priority=dict(scale=64.0, floor=1, cap=1 << 20))]
        fits.append((torch.cat(stats).cpu(), trainer.params.cpu(), trainer.m.cpu(), trainer.v.cpu(), buf.priority.cpu()))
    for a, b in zip(*fits):
        assert torch.equal(a, b)
    assert float(fits[1][0][:, 2].min()) > 0


def test_the_visit_count_form_still_equals_the_host_flavour(rows):
    dev, host = H.Env(H.net64(), DEV), H.Env(H.net64(), "cpu")
    obs, mask, v_old, z_old = rows
    for layout, inplace in ((RING, True), (BATCH, False)):
        got, exp = (H.run(e, obs, mask, v_old, z_old, 16, layout=layout, inplace=inplace, lead=1) for e in (dev, host))
        assert all(got[k].tobytes() == exp[k].tobytes() for k in exp), (layout is RING, inplace)
    assert (exp["visits"][exp["census"] >= 0].sum(1) == 16).all()
