"""gbl_train_step_weighted and gbl_replay_importance restated (test helpers): the header's additions to gbl_train_step's bit-defined
rule in numpy float32, operation by operation, on top of tests/train_restatement.py (imported, not edited); the weighted loss in torch
with autograd; and runners of the two entry points of either flavour on numpy arrays."""
import ctypes as C

import numpy as np
import torch

from gobblet_rl_amd import _native as nat
from tests import train_restatement as R

F = R.F
FLT_MAX = np.finfo(F).max
PRIO_TOP = 1 << 30
NAMES = R.NAMES + ("row_loss_out", "prio_out")


def effective(weights, B):
    """ww of the header: a NaN, a negative, a zero and +inf all count 0; None is all ones."""
    if weights is None:
        return np.ones(B, F)
    w = np.ascontiguousarray(weights, F)
    with np.errstate(invalid="ignore"):
        return np.where((w > 0) & (w <= FLT_MAX), w, F(0))


def restate_priority(lp, lv, counted, scale, floor, cap):
    """prio_out of the header from the rows' unweighted loss terms."""
    q = (lp + lv) * F(scale)
    with np.errstate(invalid="ignore"):
        small, top = ~(q > 0), q >= F(2.0 ** 30)
        k = np.where(small, 0, np.where(top, PRIO_TOP, np.where(small | top, F(0), q).astype(np.int32))).astype(np.int64)
    return np.where(counted, np.minimum(int(floor) + k, int(cap)), 0).astype(np.int32)


def restate_step(obs, mask, visits, z, hidden, params, m, v, hy, weights=None, prio=None):
    """One weighted step of the rule: (params', m', v', g, stats, row_loss (B, 2), prio_out (B,) or None), all float32 / int32.
    `prio` is (scale, floor, cap).  R.restate_step with ww folded into do and the loss terms before dh and the sums are formed."""
    B, H, P = len(obs), hidden, R.param_count(hidden)
    rows = R.restate_rows(obs, mask, visits, z, H, params, hy["value_reg"])
    ww = effective(weights, B)
    w2 = R.split(params, H)[2]
    do = ww[:, None] * rows["do"]                       # one multiply each
    acc = np.zeros((B, H), F)
    for k in range(55):
        acc = acc + do[:, k, None] * w2[:, k][None, :]
    dh = np.where((rows["pre"] > 0) & rows["counted"][:, None], acc, F(0))
    wlp, wlv = ww * rows["lp"], ww * rows["lv"]
    x = obs != 0
    always = np.ones(P + 2, bool)
    total = np.zeros(P + 2, F)
    for r0 in range(0, B, R.CHUNK):
        acc = np.zeros(P + 2, F)
        for r in range(r0, min(B, r0 + R.CHUNK)):
            h = rows["h"][r]
            term = np.concatenate([np.tile(dh[r], 117), dh[r], (h[:, None] * do[r][None, :]).reshape(-1), do[r], [wlp[r], wlv[r]]]).astype(F)
            adds = always.copy()
            adds[:117 * H] = np.repeat(x[r], H)
            acc = np.where(adds, acc + term, acc)
        total = total + acc
    N = int(rows["counted"].sum())
    M = F(max(N, 1))
    g = total[:P] / M + hy["weight_decay"] * params
    m2 = hy["beta1"] * m + (F(1) - hy["beta1"]) * g
    v2 = hy["beta2"] * v + (F(1) - hy["beta2"]) * (g * g)
    p2 = params - (hy["lr"] * (m2 / hy["bias1"])) / (np.sqrt(v2 / hy["bias2"]) + hy["eps"])
    stats = np.array([total[P] / M, total[P + 1] / M, F(N), rows["top"].max() if N else F(0)], F)
    row_loss = np.stack([rows["lp"], rows["lv"]], 1).astype(F)
    prio_out = None if prio is None else restate_priority(rows["lp"], rows["lv"], rows["counted"], *prio)
    assert all(a.dtype == F for a in (g, m2, v2, p2, stats, row_loss))
    return p2, m2, v2, g, stats, row_loss, prio_out


def restate_importance(prio, beta):
    """weights_out of the header."""
    p = np.ascontiguousarray(prio, np.int32)
    pos = p > 0
    if not pos.any():
        return np.zeros(len(p), F)
    wmin = p[pos].min()
    ratio = np.where(pos, p, wmin).astype(F) / F(wmin)
    x = F(beta) * R.log32(ratio)
    return np.where(pos, R.exp32(-x), F(0)).astype(F)


# ---- the weighted loss in torch --------------------------------------------------------------------------------------------------------
def torch_gradient(obs, mask, visits, z, hidden, params, weights, weight_decay, value_reg, dtype):
    """g of the loss sum_r ww_r (lp_r + lv_r) / M by autograd in `dtype` on the CPU, with the L2 term (R.torch_gradient, weighted)."""
    p = torch.tensor(np.asarray(params, np.float64), dtype=dtype, requires_grad=True)
    w1, b1, w2, b2 = R.split(p, hidden)
    cand = torch.ones((len(obs), 54), dtype=torch.bool) if mask is None else torch.from_numpy(mask != 0)
    vis = torch.where(cand, torch.from_numpy(visits.astype(np.int64)), torch.zeros((), dtype=torch.int64))
    S = vis.sum(1)
    counted = (torch.from_numpy(z.astype(np.int64)) != R.Z_OPEN) & (S > 0)
    ww = torch.from_numpy(effective(weights, len(obs)).astype(np.float64))[counted].to(dtype)
    x, cand, vis, S = torch.from_numpy(obs != 0)[counted].to(dtype), cand[counted], vis[counted].to(dtype), S[counted].to(dtype)
    zt = torch.from_numpy(z.astype(np.float64))[counted].to(dtype)
    out = torch.relu(x @ w1 + b1) @ w2 + b2
    logp = torch.log_softmax(out[:, :54].masked_fill(~cand, float("-inf")), 1)
    policy = -(torch.where(cand, (vis / S[:, None]) * logp.masked_fill(~cand, 0.0), torch.zeros((), dtype=dtype))).sum(1)
    value = (out[:, 54].clamp(-1, 1) - zt) ** 2 + value_reg * out[:, 54] ** 2
    n = counted.sum().to(dtype)
    ((ww * policy).sum() / n + (ww * value).sum() / n).backward()
    return (p.grad + weight_decay * p.detach()).numpy()


# ---- running the library -----------------------------------------------------------------------------------------------------------------
def run_step(lib, obs, mask, visits, z, hidden, params, m, v, hy, weights=None, prio=None, prefix="gbl_cpu_", row_loss=True, unread=(0.0, 0, 0)):
    """gbl_cpu_train_step_weighted on numpy arrays: (params', m', v', g, stats, row_loss or None, prio_out or None).  `unread`: the
    three priority scalars of a call without prio_out."""
    B, P = len(obs), R.param_count(hidden)
    obs, visits, z = np.ascontiguousarray(obs, np.int8), np.ascontiguousarray(visits, np.int16), np.ascontiguousarray(z, np.int8)
    mask = None if mask is None else np.ascontiguousarray(mask, np.int8)
    weights = None if weights is None else np.ascontiguousarray(weights, F)
    p2, m2, v2 = (np.array(a, F, copy=True) for a in (params, m, v))
    g, stats = np.full(P, np.nan, F), np.full(4, np.nan, F)
    rl = np.full((B, 2), np.nan, F) if row_loss else None
    po = None if prio is None else np.full(B, -7, np.int32)
    scale, floor, cap = unread if prio is None else prio
    ws = np.zeros(nat.lib().gbl_train_workspace_bytes(B, hidden), np.uint8)
    hs = R.hyper_struct(hy)
    rc = getattr(lib, prefix + "train_step_weighted")(
        obs.ctypes.data, None if mask is None else mask.ctypes.data, visits.ctypes.data, z.ctypes.data, B, hidden, p2.ctypes.data,
        m2.ctypes.data, v2.ctypes.data, C.addressof(hs), None if weights is None else weights.ctypes.data,
        None if rl is None else rl.ctypes.data, None if po is None else po.ctypes.data, float(scale), int(floor), int(cap), g.ctypes.data,
        stats.ctypes.data, ws.ctypes.data, ws.nbytes, None)
    assert rc == 0, getattr(lib, prefix + "last_error")()
    return p2, m2, v2, g, stats, rl, po


def run_importance(lib, prio, beta, prefix="gbl_cpu_"):
    prio = np.ascontiguousarray(prio, np.int32)
    out = np.full(len(prio), np.nan, F)
    rc = getattr(lib, prefix + "replay_importance")(prio.ctypes.data, len(prio), float(beta), out.ctypes.data, None)
    assert rc == 0, getattr(lib, prefix + "last_error")()
    return out


def same_bits(got, exp, what=""):
    for name, a, b in zip(NAMES, got, exp):
        if a is None or b is None:
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.itemsize == 4 and b.itemsize == 4, (what, name)
        bad = np.flatnonzero(a.view(np.uint32).reshape(-1) != b.view(np.uint32).reshape(-1))
        assert bad.size == 0, (what, name, bad.size, bad[:5], a.reshape(-1)[bad[:5]], b.reshape(-1)[bad[:5]])


def random_weights(B, seed, special=True):
    """Weights in (0, 4]; from 8 rows on with a 0, a denormal, -1, NaN and +inf among them (the last three count 0)."""
    rng = np.random.default_rng(seed)
    w = (4.0 - rng.uniform(0.0, 4.0, B)).astype(F)
    if special and B >= 8:
        w[[0, 3, 4, 5, 7]] = [0.0, 1e-41, -1.0, np.nan, np.inf]
    return w
