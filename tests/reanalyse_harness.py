"""What tests/test_reanalyse.py and tests/test_gpu_reanalyse.py share: one call of gbl_reanalyse / gbl_cpu_reanalyse on pitched, guarded
buffers (tests/tb_targets_harness.py's Buf: a non-zero lead, junk in the padding and around the rows, every byte outside the rows
checked), the row sources, and the expectation from tests/reanalyse_restatement.py.  A plain module."""
import ctypes as C

import numpy as np
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as ER
from tests import reanalyse_restatement as RR
from tests.tb_targets_harness import BATCH, JUNK, RING, Buf

DENSE = (("root_value", np.int32, 1), ("root_priors", np.uint8, 54), ("action", np.int32, 1), ("nodes", np.int32, 1), ("drift", np.int32, 1),
         ("census", np.int8, 1))
ALL = tuple(k for k, _, _ in DENSE)
EXPLORE = 16


class Env:
    """One flavour with one network: "cpu" (host arrays) or a device name (the arrays are uploaded, the evaluator's too)."""

    def __init__(self, net, device="cpu"):
        self.net, self.device, self.host = net, device, device == "cpu"
        self.L, self.prefix = (nat.cpu_raw(), "gbl_cpu_") if self.host else (nat.lib(), "gbl_")
        self.arrays = None if self.host else [torch.from_numpy(a).to(device) for a in (net.w1, net.b1, net.w2, net.b2)]
        self.upload = None if self.host else (lambda raw: torch.from_numpy(raw).to(device))
        self.stream = None if self.host else nat.current_stream(device)

    def error(self):
        return getattr(self.L, self.prefix + "last_error")()

    def evaluator(self):
        n = self.net
        return G.GobbletEvaluator(n.w1, n.b1, n.w2, n.b2, n.shift1, n.shift_p, n.shift_v, device=self.device)


def run(env, obs, mask=None, visits_old=None, z_old=None, iterations=8, explore=EXPLORE, layout=BATCH, inplace=True, keep=ALL, lead=0,
        give_visits_out=True):
    """One call on fresh buffers.  visits_old / z_old: visits_in / z_in (None: NULL).  inplace: visits_out is visits_in's own pointer
    (where there is one); otherwise the output rows start as junk.  The ring layout keeps z inside the mask's rows (byte 54 of 64), as
    ring_meta does.  Returns "visits" and the kept dense outputs; every input row, every padding byte and every output not asked for
    is checked to be untouched."""
    n = len(obs)
    up, ring = env.upload, layout is RING
    lead2 = lead & ~1                                                  # (int16 rows: the device flavour wants them 2-byte aligned)
    lead4 = lead & ~3
    b_obs = Buf(obs, layout["obs"], lead, up)
    if ring:
        meta = np.full((n, 64), JUNK, np.int8)
        meta[:, :54] = 0 if mask is None else mask
        meta[:, 54] = JUNK if z_old is None else z_old
        b_meta = Buf(meta, 64, lead, up)
        mask_ptr, z_ptr = (None if mask is None else b_meta.ptr), (None if z_old is None else b_meta.ptr + 54)
    else:
        b_mask = None if mask is None else Buf(mask, layout["mask"], 3 * lead, up)
        b_z = None if z_old is None else Buf(np.asarray(z_old, np.int8).reshape(n, 1), layout["z"], 5 * lead, up)
        mask_ptr, z_ptr = (None if b_mask is None else b_mask.ptr), (None if b_z is None else b_z.ptr)
    b_vin = None if visits_old is None else Buf(np.asarray(visits_old, np.int16), layout["visits"], lead2, up)
    b_vout = b_vin if (inplace and b_vin is not None) else Buf(np.full((n, 54), 0x5A5A, np.int16), layout["visits"], lead2 + 2 * (lead != 0), up)
    dense = {k: Buf(np.full((n, row), 0x5A5A5A5A if dt == np.int32 else JUNK, dt), row, lead4 if dt == np.int32 else lead, up)
             for k, dt, row in DENSE}
    ev = env.net.struct(env.arrays)
    rc = getattr(env.L, env.prefix + "reanalyse")(
        C.addressof(ev), iterations, explore, b_obs.ptr, layout["obs"], mask_ptr, layout["mask"], None if b_vin is None else b_vin.ptr,
        b_vout.ptr if give_visits_out else None, layout["visits"], z_ptr, layout["z"], *[dense[k].ptr if k in keep else None for k in ALL],
        n, env.stream)
    assert rc == 0, env.error()
    if not env.host:
        torch.cuda.synchronize()
    got = {"visits": b_vout.rows()}
    assert np.array_equal(b_obs.rows(), obs), "the observation rows were written"
    if ring:
        assert np.array_equal(b_meta.rows(), meta), "a byte of ring_meta was written"
    else:
        assert b_mask is None or np.array_equal(b_mask.rows(), mask)
        assert b_z is None or np.array_equal(b_z.rows()[:, 0], z_old)
    if b_vin is not None and b_vout is not b_vin:
        assert np.array_equal(b_vin.rows(), visits_old)
    if not give_visits_out:
        assert np.array_equal(got["visits"], b_vout.before[b_vout.payload].view(np.int16).reshape(n, 54)), "visits_out was NULL and rows were written"
    for k, dt, row in DENSE:
        rows = dense[k].rows()
        if k in keep:
            got[k] = rows if row > 1 else rows[:, 0]
        else:
            assert (rows.view(np.uint8) == JUNK).all(), k
    return got


def check(got, exp, visits_before, what=""):
    """got against the restatement's outputs; a skipped row must still hold visits_before (an array, or a scalar for a junk fill)."""
    vb = np.broadcast_to(np.asarray(visits_before, np.int16), got["visits"].shape)
    assert np.array_equal(got["visits"], np.where(exp["written"][:, None], exp["visits"], vb)), (what, "visits")
    for k in ALL:
        if k in got:
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5])


# ---- row sources ------------------------------------------------------------------------------------------------------------------
def selfplay_ring(net, device="cpu", boards=64, plies=12, iterations=8, sample_plies=4, capacity=1024, seed=7, explore=EXPLORE, **kw):
    """An un-noised evaluator-against-evaluator window appended to a fresh ring: (buffer, evaluator)."""
    n = net
    ev = G.GobbletEvaluator(n.w1, n.b1, n.w2, n.b2, n.shift1, n.shift_p, n.shift_v, device=device)
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=iterations, sample_plies=sample_plies, explore=explore))
    env.outcome_targets(traj)
    buf = G.ReplayBuffer(capacity, device, **kw)
    buf.append(env, traj, tag=1)
    return buf, ev


def ring_rows(buf):
    live = buf.size
    return tuple(t[:live].cpu().numpy().copy() for t in (buf.observation, buf.action_mask, buf.visits, buf.z))


def random_rows(n, seed):
    """Masked-random full-inventory positions after 1 .. 12 plies, both movers, with their legal masks."""
    from tests.tb_targets_harness import legal_mask, random_play_rows
    obs, st, tm = random_play_rows(2 * n, (1, 2, 3, 5, 8, 12), seed)   # (some games are over by then: ask for more, keep n)
    pick = np.random.default_rng(seed).permutation(len(obs))[:n]
    assert len(pick) == n and set(tm[pick].tolist()) == {0, 1}
    return obs[pick], legal_mask(st[pick], tm[pick])


def make_rows(net):
    """The rows of both test modules: the live rows of a 64-board, 12-ply self-play ring, then 32 masked-random positions with search-like
    old visits, some rows skipped (z = GBL_Z_OPEN).  (obs, mask, visits_old, z_old)."""
    buf, _ = selfplay_ring(net)
    obs, mask, visits, z = ring_rows(buf)
    r_obs, r_mask = random_rows(32, 17)
    rng = np.random.default_rng(18)
    r_vis = (rng.integers(0, 40, (32, 54)) * (rng.random((32, 54)) < 0.3)).astype(np.int16) * (r_mask != 0)
    r_z = rng.choice(np.array([-1, 0, 1, nat.Z_OPEN], np.int8), 32, p=[0.3, 0.2, 0.3, 0.2])
    return np.concatenate([obs, r_obs]), np.concatenate([mask, r_mask]), np.concatenate([visits, r_vis]), np.concatenate([z, r_z])


def net64():
    return ER.random_net(64, 69)
