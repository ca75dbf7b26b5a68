"""What tests/test_reanalyse_gumbel.py and tests/test_gpu_reanalyse_gumbel.py share: one call of gbl_reanalyse_gumbel /
gbl_cpu_reanalyse_gumbel on pitched, guarded buffers (tests/reanalyse_harness.py's layout: tests/tb_targets_harness.py's Buf, a non-zero
lead, junk in the padding and around the rows, every byte outside the rows checked), and the row sources.  A plain module."""
import ctypes as C

import numpy as np
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import reanalyse_harness as H
from tests.tb_targets_harness import BATCH, JUNK, RING, Buf

DENSE = H.DENSE + (("gumbel", np.int16, 54),)
ALL = tuple(k for k, _, _ in DENSE)
EXPLORE = H.EXPLORE
RULE = (16, 1, 50, 23)   # considered, gumbel_noise, visit_offset, scale: the defaults of gumbel=dict()


def run(env, obs, mask=None, visits_old=None, z_old=None, iterations=16, rule=RULE, seed=0, env_base=0, call=0, explore=EXPLORE, layout=BATCH,
        inplace=True, keep=ALL, lead=0, give_visits_out=True):
    """tests/reanalyse_harness.py's run for the Gumbel entry point: one call on fresh buffers, returns "visits" and the kept dense
    outputs; every input row, every padding byte and every output not asked for is checked to be untouched."""
    n = len(obs)
    up, ring = env.upload, layout is RING
    lead2, lead4 = lead & ~1, lead & ~3
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
    fill = {np.int32: 0x5A5A5A5A, np.int16: 0x5A5A}
    dense = {k: Buf(np.full((n, row), fill.get(dt, JUNK), dt), row, lead4 if dt == np.int32 else lead2 if dt == np.int16 else lead, up)
             for k, dt, row in DENSE}
    ev = env.net.struct(env.arrays)
    rc = getattr(env.L, env.prefix + "reanalyse_gumbel")(
        C.addressof(ev), iterations, explore, *rule, seed, env_base, call, b_obs.ptr, layout["obs"], mask_ptr, layout["mask"],
        None if b_vin is None else b_vin.ptr, b_vout.ptr if give_visits_out else None, layout["visits"], z_ptr, layout["z"],
        *[dense[k].ptr if k in keep else None for k in ALL], n, env.stream)
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
def gumbel_ring(net, device="cpu", boards=24, plies=8, iterations=16, capacity=512, seed=7, explore=EXPLORE, rule=RULE, **kw):
    """A Gumbel self-play window (both sides by the rule) appended to a fresh ring: (buffer, evaluator).  The rows are target rows."""
    ev = G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, net.shift1, net.shift_p, net.shift_v, device=device)
    env = G.BatchedGobblet(boards, device, auto_reset=True, seed=seed, track_turn=True)
    gum = dict(considered=rule[0], noise=bool(rule[1]), visit_offset=rule[2], scale=rule[3])
    traj = env.collect(plies, policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=iterations, explore=explore, gumbel=gum))
    env.outcome_targets(traj)
    buf = G.ReplayBuffer(capacity, device, **kw)
    buf.append(env, traj, tag=1)
    return buf, ev


def planted_rows():
    """A small set with every kind of row: masked-random full-inventory positions of both movers under their legal masks, then rows
    with a restricting mask, 27 / 3 / 2 / 1 / 0 candidates, the empty board (all 54 actions) and skipped rows.
    (obs, mask, visits_old, z_old)."""
    obs, mask = H.random_rows(20, 23)
    obs, mask = obs.copy(), mask.copy()
    rng = np.random.default_rng(24)
    cand = [np.flatnonzero(m) for m in mask]
    assert all(len(c) > 2 for c in cand) and len(cand[13]) > 27
    mask[3, cand[3][len(cand[3]) // 2:]] = 0                    # a restricting mask
    mask[4, cand[4][2:]] = 0                                    # 2 candidates
    mask[5, cand[5][1:]] = 0                                    # 1
    mask[6] = 0                                                 # 0
    obs[7], mask[7] = 0, 1                                      # the empty board: all 54 actions are candidates
    mask[13, cand[13][27:]] = 0                                 # 27 candidates
    mask[8, cand[8][3:]] = 0                                    # 3 candidates: one halving at most
    v_old = (rng.integers(0, 200, (20, 54)) * (rng.random((20, 54)) < 0.4)).astype(np.int16) * (mask != 0)
    v_old[9] = 0                                                # no old visits
    v_old[10] = -5                                              # ... or only negative ones
    v_old[11] = 32767                                           # So = 54 * 32767
    z_old = rng.choice(np.array([-1, 0, 1], np.int8), 20)
    z_old[[2, 12, 19]] = nat.Z_OPEN                             # skipped, the last row among them
    return obs, mask, v_old, z_old
