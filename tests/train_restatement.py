"""gbl_train_step restated (test helpers): the header's bit-defined rule in numpy float32, operation by operation -- vectorised over
rows or over parameters, never over an axis the rule sums in a stated order --, the same loss in torch with autograd (float64: the
reference; float32: the yardstick), and builders of batches by hand and through env.training_batch on the host flavour."""
import ctypes as C

import numpy as np
import torch

from gobblet_rl_amd import _native as nat

F = np.float32
Z_OPEN = -128
CHUNK = 64
HYPER = dict(lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-4, value_reg=1e-2)


def fx(text):
    return F(float.fromhex(text))


LOG2E, LN2_HI, LN2_LO = fx("0x1.715476p+0"), fx("0x1.62e4p-1"), fx("0x1.7f7d1cp-20")
EXP_C = [fx(t) for t in ("0x1.a01a02p-13", "0x1.6c16c2p-10", "0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3", "0x1p-1")]  # C7 .. C2
LOG_D = [fx(t) for t in ("0x1.c71c72p-3", "0x1.24924ap-2", "0x1.99999ap-2", "0x1.555556p-1")]  # D4 .. D1


def pow2(n):
    return ((n + 127).astype(np.uint32) << np.uint32(23)).view(F)


def exp32(x):
    """EXP of the header on a float32 array."""
    x = np.ascontiguousarray(x, F)
    x = np.where(x >= F(-110), x, F(-110))
    x = np.where(x <= F(0), x, F(0))
    t = x * LOG2E
    n = (t - F(0.5)).astype(np.int32)   # (astype truncates toward zero, as the cast does)
    fn = n.astype(F)
    r = (x - fn * LN2_HI) - fn * LN2_LO
    q = EXP_C[0]
    for c in EXP_C[1:]:
        q = q * r
        q = q + c
    y = r * r
    y = y * q
    y = y + r
    y = y + F(1)
    n1 = n >> 1
    n2 = n - n1
    return (y * pow2(n1)) * pow2(n2)


def log32(s):
    """LOG of the header on a float32 array of values >= 1."""
    u = np.ascontiguousarray(s, F).view(np.uint32)
    e = (u >> np.uint32(23)).astype(np.int32) - 127
    mant = u & np.uint32(0x7FFFFF)
    upper = mant > 0x3504F3
    e = e + upper
    w = (mant | np.where(upper, np.uint32(0x3F000000), np.uint32(0x3F800000))).astype(np.uint32).view(F)
    f = w - F(1)
    q = f / (F(2) + f)
    y = q * q
    R = LOG_D[0]
    for d in LOG_D[1:]:
        R = R * y
        R = R + d
    R = R * y
    hf = (F(0.5) * f) * f
    T = q * (hf + R)
    dk = e.astype(F)
    return (((T + dk * LN2_LO) - hf) + f) + dk * LN2_HI


def param_count(hidden):
    return 173 * hidden + 55


def split(params, hidden):
    a, b, c = 117 * hidden, 118 * hidden, 173 * hidden
    return params[:a].reshape(117, hidden), params[a:b], params[b:c].reshape(hidden, 55), params[c:]


def hyper_at(t, **kw):
    """The hyper-parameters of step t (1, 2, ...) as float32, the bias corrections computed in double as the caller must."""
    h = dict(HYPER, **kw)
    h["bias1"], h["bias2"] = 1.0 - h["beta1"] ** t, 1.0 - h["beta2"] ** t
    return {k: F(v) for k, v in h.items()}


def restate_rows(obs, mask, visits, z, hidden, params, value_reg):
    """Forward and backward of every row: dict of h, dh (B, H), do (B, 55), lp, lv, top (B,), counted (B,) bool."""
    B, H = len(obs), hidden
    w1, b1, w2, b2 = split(params, H)
    x = obs != 0
    cand = np.ones((B, 54), bool) if mask is None else mask != 0
    vis = visits.astype(np.int32)
    S = np.where(cand, vis, 0).sum(1)
    counted = (z != Z_OPEN) & (S > 0)
    pre = np.tile(b1, (B, 1))
    for f in range(117):
        pre = np.where(x[:, f, None], pre + w1[f][None, :], pre)
    h = np.where(pre > 0, pre, F(0))
    o = np.tile(b2, (B, 1))
    for j in range(H):
        o = o + h[:, j, None] * w2[j][None, :]
    mx, started = np.zeros(B, F), np.zeros(B, bool)
    for a in range(54):
        take = cand[:, a] & (~started | (o[:, a] > mx))
        mx = np.where(take, o[:, a], mx)
        started |= cand[:, a]
    d = o[:, :54] - mx[:, None]
    e = np.where(cand, exp32(d), F(0))
    s = np.zeros(B, F)
    for a in range(54):
        s = np.where(cand[:, a], s + e[:, a], s)
    s = np.where(counted, s, F(1))          # (uncounted rows are zeroed below: keep their arithmetic quiet)
    L = log32(s)
    t = vis.astype(F) / np.where(counted, S, 1).astype(F)[:, None]
    do = np.zeros((B, 55), F)
    do[:, :54] = np.where(cand, e / s[:, None] - t, F(0))
    term = t * (L[:, None] - d)
    lp = np.zeros(B, F)
    for a in range(54):
        lp = np.where(cand[:, a], lp + term[:, a], lp)
    v = o[:, 54]
    c = np.where(v < F(-1), F(-1), np.where(v > F(1), F(1), v))
    u = c - z.astype(F)
    lv = u * u + value_reg * (v * v)
    do[:, 54] = F(2) * np.where((v > F(-1)) & (v < F(1)), u, F(0)) + F(2) * (value_reg * v)
    acc = np.zeros((B, H), F)
    for k in range(55):
        acc = acc + do[:, k, None] * w2[:, k][None, :]
    dh = np.where(pre > 0, acc, F(0))
    keep = counted[:, None]
    h, dh, do = np.where(keep, h, F(0)), np.where(keep, dh, F(0)), np.where(keep, do, F(0))
    lp, lv = np.where(counted, lp, F(0)), np.where(counted, lv, F(0))
    return dict(h=h, dh=dh, do=do, lp=lp, lv=lv, top=h.max(1), counted=counted, o=o, pre=pre)


def restate_step(obs, mask, visits, z, hidden, params, m, v, hy):
    """One step of the rule: (params', m', v', g, stats), all float32."""
    B, H, P = len(obs), hidden, param_count(hidden)
    rows = restate_rows(obs, mask, visits, z, H, params, hy["value_reg"])
    x = obs != 0
    # SUM of the header for all P elements and the two loss terms at once: serial over the rows of a chunk and over the chunks
    always = np.ones(P + 2, bool)
    total = np.zeros(P + 2, F)
    for r0 in range(0, B, CHUNK):
        acc = np.zeros(P + 2, F)
        for r in range(r0, min(B, r0 + CHUNK)):
            h, dh, do = rows["h"][r], rows["dh"][r], rows["do"][r]
            term = np.concatenate([np.tile(dh, 117), dh, (h[:, None] * do[None, :]).reshape(-1), do, [rows["lp"][r], rows["lv"][r]]]).astype(F)
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
    assert all(a.dtype == F for a in (g, m2, v2, p2, stats))
    return p2, m2, v2, g, stats


# ---- the same loss in torch ------------------------------------------------------------------------------------------------------------
def torch_gradient(obs, mask, visits, z, hidden, params, weight_decay, value_reg, dtype):
    """(g, policy loss, value loss) of the header's loss by autograd in `dtype` on the CPU, g with the L2 term."""
    p = torch.tensor(np.asarray(params, np.float64), dtype=dtype, requires_grad=True)
    w1, b1, w2, b2 = split(p, hidden)
    cand = torch.ones((len(obs), 54), dtype=torch.bool) if mask is None else torch.from_numpy(mask != 0)
    vis = torch.where(cand, torch.from_numpy(visits.astype(np.int64)), torch.zeros((), dtype=torch.int64))
    S = vis.sum(1)
    counted = (torch.from_numpy(z.astype(np.int64)) != Z_OPEN) & (S > 0)
    if not bool(counted.any()):
        return (weight_decay * p.detach()).numpy(), 0.0, 0.0
    x, cand, vis, S = torch.from_numpy(obs != 0)[counted].to(dtype), cand[counted], vis[counted].to(dtype), S[counted].to(dtype)
    zt = torch.from_numpy(z.astype(np.float64))[counted].to(dtype)
    out = torch.relu(x @ w1 + b1) @ w2 + b2
    logp = torch.log_softmax(out[:, :54].masked_fill(~cand, float("-inf")), 1)
    policy = -(torch.where(cand, (vis / S[:, None]) * logp.masked_fill(~cand, 0.0), torch.zeros((), dtype=dtype))).sum(1)
    value = (out[:, 54].clamp(-1, 1) - zt) ** 2 + value_reg * out[:, 54] ** 2
    n = counted.sum().to(dtype)
    (policy.sum() / n + value.sum() / n).backward()
    g = p.grad + weight_decay * p.detach()
    return g.numpy(), float(policy.detach().sum() / n), float(value.detach().sum() / n)


# ---- running the library -----------------------------------------------------------------------------------------------------------------
def hyper_struct(hy):
    return nat.TrainHyper(*[float(hy[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "value_reg", "bias1", "bias2")])


def run_step(lib, obs, mask, visits, z, hidden, params, m, v, hy, prefix="gbl_cpu_", grad=True):
    """gbl_cpu_train_step on numpy arrays: (params', m', v', g or None, stats); the inputs are left alone."""
    B, P = len(obs), param_count(hidden)
    obs, visits, z = np.ascontiguousarray(obs, np.int8), np.ascontiguousarray(visits, np.int16), np.ascontiguousarray(z, np.int8)
    mask = None if mask is None else np.ascontiguousarray(mask, np.int8)
    p2, m2, v2 = (np.array(a, F, copy=True) for a in (params, m, v))
    g, stats = (np.full(P, np.nan, F) if grad else None), np.full(4, np.nan, F)
    ws = np.zeros(nat.lib().gbl_train_workspace_bytes(B, hidden), np.uint8)
    hs = hyper_struct(hy)
    rc = getattr(lib, prefix + "train_step")(obs.ctypes.data, None if mask is None else mask.ctypes.data, visits.ctypes.data, z.ctypes.data,
                                             B, hidden, p2.ctypes.data, m2.ctypes.data, v2.ctypes.data, C.addressof(hs),
                                             None if g is None else g.ctypes.data, stats.ctypes.data, ws.ctypes.data, ws.nbytes, None)
    assert rc == 0, getattr(lib, prefix + "last_error")()
    return p2, m2, v2, g, stats


NAMES = ("params", "adam_m", "adam_v", "grad_out", "stats_out")


def same_bits(got, exp, what=""):
    for name, a, b in zip(NAMES, got, exp):
        if a is None or b is None:
            continue
        a, b = np.asarray(a, F), np.asarray(b, F)
        bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
        assert bad.size == 0, (what, name, bad.size, bad[:5], a[bad[:5]], b[bad[:5]])


# ---- batches -------------------------------------------------------------------------------------------------------------------------------
def init_params(hidden, seed):
    """A network of from_float's shapes, off any grid, with hidden units on both sides of zero."""
    rng = np.random.default_rng(seed)
    w1 = rng.uniform(-1, 1, (117, hidden)) / np.sqrt(21.0)
    w2 = rng.uniform(-1, 1, (hidden, 55)) / np.sqrt(hidden)
    return np.concatenate([w1.reshape(-1), rng.uniform(-0.3, 0.3, hidden), w2.reshape(-1), rng.uniform(-0.5, 0.5, 55)]).astype(F)


def random_batch(B, seed, with_mask=True):
    """(obs, mask or None, visits, z): about 18 set bytes per observation, candidate sets of 1 .. 54 actions, visits only inside the
    mask plus junk outside it (which the rule must not read), every z value, and -- from 4 rows on -- one open row and one row without visits."""
    rng = np.random.default_rng(seed)
    obs = (rng.random((B, 117)) < 0.15).astype(np.int8)
    mask = (rng.random((B, 54)) < rng.uniform(0.05, 1.0, (B, 1))).astype(np.int8)
    mask[np.arange(B), rng.integers(0, 54, B)] = 1
    visits = (rng.integers(0, 200, (B, 54)) * (rng.random((B, 54)) < 0.6)).astype(np.int16)
    visits[np.arange(B), mask.argmax(1)] += 1
    z = rng.integers(-1, 2, B).astype(np.int8)
    if with_mask:
        visits = np.where(mask != 0, visits, rng.integers(-50, 50, (B, 54))).astype(np.int16)
    else:
        mask = None
    if B >= 4:
        z[1] = Z_OPEN
        visits[2] = 0
    return obs, mask, visits, z


def window_batches(boards, plies, batch, calls, seed=17, symmetries="all"):
    """`calls` batches of `batch` samples drawn by env.training_batch (host flavour) from a tree-vs-tree window: list of
    (obs, mask, visits, z) numpy tuples, and (env, traj)."""
    import gobblet_rl_amd as G
    env = G.BatchedGobblet(boards, "cpu", auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("tree", "tree"), search=dict(iterations=8, playouts=2, sample_plies=4))
    env.outcome_targets(traj)
    out = []
    for c in range(calls):
        b = env.training_batch(traj, batch, symmetries=symmetries, call=c)
        out.append(tuple(b[k].numpy().copy() for k in ("observation", "action_mask", "visits", "z")))
    return out, (env, traj)


# ---- edge batches: (obs, mask, visits, z, hidden, params, hyper overrides), shared by the host and the device tests ------------------------
def _fresh(hidden):
    return init_params(hidden, hidden)


def edge_none_counted():
    obs, mask, visits, z = random_batch(5, 1)
    z[:] = Z_OPEN
    z[3], visits[3] = 1, 0                      # (one row with an outcome and no visits: not counted either)
    return obs, mask, visits, z, 64, _fresh(64), {}


def edge_open_rows():
    obs, mask, visits, z = random_batch(40, 2)
    z[[5, 17, 39]] = Z_OPEN
    return obs, mask, visits, z, 64, _fresh(64), {}


def edge_one_candidate():
    obs = random_batch(1, 3)[0]
    mask, visits, z = np.zeros((1, 54), np.int8), np.full((1, 54), 9, np.int16), np.array([1], np.int8)
    mask[0, 31] = 1
    return obs, mask, visits, z, 64, _fresh(64), {}


def edge_logits_200_apart():
    obs, _, visits, z = random_batch(3, 4, with_mask=False)
    p = _fresh(64)
    _, _, w2, b2 = split(p, 64)
    w2[:, :2] = 0
    b2[0], b2[1] = 120.0, -80.0
    visits[:] = 0
    visits[:, 1] = 5                            # all the visits on the action whose probability underflows
    return obs, None, visits, z, 64, p, {}


def edge_value(value):
    obs, mask, visits, z = random_batch(1, 5)
    z[0] = 1
    p = _fresh(64)
    split(p, 64)[2][:, 54] = 0
    split(p, 64)[3][54] = value
    return obs, mask, visits, z, 64, p, {}


def edge_hidden_zero():
    obs, mask, visits, z = random_batch(9, 6)
    p = _fresh(64)
    w1, b1, _, _ = split(p, 64)
    w1[:, 7], b1[7] = 0, 0
    return obs, mask, visits, z, 64, p, {}


def edge_no_regularisers(**off):
    obs, mask, visits, z = random_batch(70, 8)
    return obs, mask, visits, z, 128, _fresh(128), off


VALUES = (0.5, -0.999, 1.0, -1.0, 1.5, -2.0)
EDGES = {"none counted": edge_none_counted, "open rows": edge_open_rows, "one candidate": edge_one_candidate,
         "logits 200 apart": edge_logits_200_apart, "hidden unit at 0": edge_hidden_zero,
         "weight_decay 0": lambda: edge_no_regularisers(weight_decay=0.0), "value_reg 0": lambda: edge_no_regularisers(value_reg=0.0),
         "both 0": lambda: edge_no_regularisers(weight_decay=0.0, value_reg=0.0),
         **{"value %g" % x: (lambda x=x: edge_value(x)) for x in VALUES}}
