"""The "Board symmetries" paragraph and the draw rule of gbl_training_batch (include/gobblet_hip.h) restated in numpy from the header's
text: sigma from the (r, c) formula, the swaps from the bit layout, the generator from oracle.philox4x32_10.  No code or table shared
with the library (test infrastructure).  Also the windows and the calls through a library handle that the CPU and the GPU tests share."""
import functools

import numpy as np

import oracle

N_SYM, ATTEMPTS, Z_OPEN, STREAM = 512, 16, -128, 5
ROWS = ("state", "obs", "mask", "visits", "priors", "actions")
DTYPES = {"state": np.int8, "obs": np.int8, "mask": np.int8, "visits": np.int16, "priors": np.uint8, "actions": np.int32}
WIDTHS = {"state": 27, "obs": 117, "mask": 54, "visits": 54, "priors": 54}
BATCH_OUT = ("obs", "mask", "visits", "z", "index", "sym")


def sigma(s):
    """sigma(p) for p = 0..8: flip first (c <- 2 - c), then rot times (r, c) <- (c, 2 - r)."""
    out = []
    for p in range(9):
        r, c = p // 3, p % 3
        if (s >> 2) & 1:
            c = 2 - c
        for _ in range(s & 3):
            r, c = c, 2 - r
        out.append(3 * r + c)
    return out


def tau(s, m):
    """tau_m on piece numbers 0..6 (0 stays): bit 3 + k swaps player_1's 2k+1 <-> 2k+2, bit 6 + k player_2's."""
    t = list(range(7))
    for k in range(3):
        if (s >> ((6 if m else 3) + k)) & 1:
            t[2 * k + 1], t[2 * k + 2] = 2 * k + 2, 2 * k + 1
    return t


@functools.lru_cache(maxsize=None)
def tables():
    """For every code: where each element of a row GOES.  state_to (512, 27), state_val (512, 13) indexed by v + 6, act_to (512, 2, 54),
    obs_to (512, 2, 117)."""
    state_to, state_val = np.zeros((N_SYM, 27), np.int64), np.zeros((N_SYM, 13), np.int8)
    act_to, obs_to = np.zeros((N_SYM, 2, 54), np.int64), np.zeros((N_SYM, 2, 117), np.int64)
    for s in range(N_SYM):
        sg, t = sigma(s), (tau(s, 0), tau(s, 1))
        for lvl in range(3):
            for p in range(9):
                state_to[s, 9 * lvl + p] = 9 * lvl + sg[p]
        for v in range(-6, 7):
            state_val[s, v + 6] = t[0][v] if v > 0 else -t[1][-v] if v < 0 else 0
        for m in range(2):
            for a in range(54):
                act_to[s, m, a] = 9 * (t[m][a // 9 + 1] - 1) + sg[a % 9]
            for p in range(9):
                for ch in range(13):
                    to = t[m][ch + 1] - 1 if ch < 6 else 6 + t[1 - m][ch - 6 + 1] - 1 if ch < 12 else 12
                    obs_to[s, m, 13 * p + ch] = 13 * sg[p] + to
    for a in (state_to, state_val, act_to, obs_to):
        a.setflags(write=False)
    return state_to, state_val, act_to, obs_to


def _scatter(rows, to):
    out = np.empty_like(rows)
    np.put_along_axis(out, to, rows, axis=1)
    return out


def apply(sym, agent=None, **rows):
    """The images of the rows (keys of ROWS; obs as (n, 117)) under the per-board codes `sym` (only their low 9 bits count)."""
    state_to, state_val, act_to, obs_to = tables()
    s = np.asarray(sym).astype(np.int64) & 511
    m = None if agent is None else (np.asarray(agent) != 0).astype(np.int64)
    out = {}
    for k, r in rows.items():
        if k == "state":
            inside = np.abs(r.astype(np.int64)) <= 6
            val = np.where(inside, state_val[s[:, None], np.clip(r.astype(np.int64), -6, 6) + 6], r).astype(np.int8)
            out[k] = _scatter(val, state_to[s])
        elif k == "obs":
            out[k] = _scatter(r, obs_to[s, m])
        elif k == "actions":
            a = r.astype(np.int64)
            ok = (a >= 0) & (a < 54)
            out[k] = np.where(ok, act_to[s, m, np.clip(a, 0, 53)], a).astype(np.int32)
        else:
            out[k] = _scatter(r, act_to[s, m])
    return out


def run_apply(lib, sym, agent=None, prefix="gbl_cpu_", **rows):
    """gbl_symmetry_apply on host arrays through a raw handle; sym: an int (sym_all) or an int16 array.  Outputs pre-filled with junk."""
    n = len(next(iter(rows.values())))
    ins = {k: np.ascontiguousarray(v, DTYPES[k]) for k, v in rows.items()}
    outs = {k: np.full_like(v, 77) for k, v in ins.items()}
    codes = None if np.isscalar(sym) else np.ascontiguousarray(sym, np.int16)
    ag = None if agent is None else np.ascontiguousarray(agent, np.int8)
    pairs = []
    for k in ROWS:
        pairs += [ins[k].ctypes.data if k in ins else None, outs[k].ctypes.data if k in outs else None]
    rc = getattr(lib, prefix + "symmetry_apply")(None if codes is None else codes.ctypes.data, int(sym) if codes is None else 0,
                                                 None if ag is None else ag.ctypes.data, *pairs, n, None)
    assert rc == 0, getattr(lib, prefix + "last_error")()
    return outs


# ---- gbl_training_batch -----------------------------------------------------------------------------------------------------------
def cell(t, b, ply_stride, tile_stride):
    return t * ply_stride + (b // 64) * tile_stride + b % 64


def window_of(traj, n):
    """A collected window (BatchedGobblet.collect + outcome_targets on the host flavour) as flat numpy arrays over the cells."""
    f = traj["_full"]
    w = {"obs": f["observation"].reshape(-1, 117), "mask": f["action_mask"].reshape(-1, 54), "visits": f["visits"].reshape(-1, 54),
         "z": f["z"].reshape(-1), "done": f["done"].reshape(-1), "mover": f["mover"].reshape(-1)}
    w = {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in w.items()}
    w.update(n=n, plies=traj["_plies"], ply_stride=traj["_ply_stride"], tile_stride=traj["_tile_stride"])
    return w


def valid_cells(w):
    """bool (plies, n): the cells gbl_training_batch may return (row 0 is never valid)."""
    t, b = np.meshgrid(np.arange(w["plies"]), np.arange(w["n"]), indexing="ij")
    at = cell(t, b, w["ply_stride"], w["tile_stride"])
    prev = cell(np.maximum(t - 1, 0), b, w["ply_stride"], w["tile_stride"])
    ok = (w["z"][at] != Z_OPEN) & (w["done"][prev] == 0) & (w["visits"][at].astype(np.int64).sum(-1) > 0)
    ok[0] = False
    return ok


def training_batch(w, batch, sym_mask, seed, sample_base, call):
    """The outputs of gbl_training_batch by the header's rule, as a dict over BATCH_OUT, and the number of failed samples."""
    ok = valid_cells(w)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    out = {"obs": np.zeros((batch, 117), np.int8), "mask": np.zeros((batch, 54), np.int8), "visits": np.zeros((batch, 54), np.int16),
           "z": np.full(batch, Z_OPEN, np.int8), "index": np.full((batch, 2), -1, np.int32), "sym": np.zeros(batch, np.int16)}
    take = np.full((batch, 3), -1, np.int64)  # (t, b, s) of the samples that found a cell
    for j in range(batch):
        ident = sample_base + j
        for i in range(ATTEMPTS):
            w0, w1, w2, _ = (int(x) for x in oracle.philox4x32_10([ident & 0xFFFFFFFF, (ident >> 32) & 0xFFFFFFFF, 16 * call + i, STREAM], key))
            t, b = 1 + ((w0 * (w["plies"] - 1)) >> 32), (w1 * w["n"]) >> 32
            if ok[t, b]:
                take[j] = t, b, w2 & sym_mask
                break
    got = np.flatnonzero(take[:, 0] >= 0)
    t, b, s = take[got].T
    at, prev = cell(t, b, w["ply_stride"], w["tile_stride"]), cell(t - 1, b, w["ply_stride"], w["tile_stride"])
    m = w["mover"][at]
    img = apply(s, m, obs=w["obs"][prev], mask=w["mask"][prev], visits=w["visits"][at])
    for k in ("obs", "mask", "visits"):
        out[k][got] = img[k]
    out["z"][got], out["sym"][got] = w["z"][at], s
    out["index"][got] = np.stack([t, b], 1)
    return out, batch - len(got)


def run_batch(lib, w, batch, sym_mask, seed, sample_base, call, prefix="gbl_cpu_", canary=0):
    """gbl_training_batch on a numpy window through a raw handle: dict over BATCH_OUT, pre-filled with junk."""
    out = {"obs": np.full((batch + canary, 117), 77, np.int8), "mask": np.full((batch + canary, 54), 77, np.int8),
           "visits": np.full((batch + canary, 54), 7777, np.int16), "z": np.full(batch + canary, 77, np.int8),
           "index": np.full((batch + canary, 2), 7777, np.int32), "sym": np.full(batch + canary, 7777, np.int16)}
    rc = getattr(lib, prefix + "training_batch")(
        *[w[k].ctypes.data for k in ("obs", "mask", "visits", "z", "done", "mover")], w["n"], w["plies"], w["ply_stride"], w["tile_stride"],
        batch, sym_mask, seed, sample_base, call, *[out[k].ctypes.data for k in BATCH_OUT], None)
    assert rc == 0, getattr(lib, prefix + "last_error")()
    return out


def same_batch(got, exp, batch=None):
    for k in BATCH_OUT:
        g, e = (got[k], exp[k]) if batch is None else (got[k][:batch], exp[k][:batch])
        assert g.dtype == e.dtype and np.array_equal(g, e), (k, np.argwhere(g != e)[:5])


WINDOWS = ((200, 12, "time"), (65, 9, "time"), (200, 12, "tile"))  # (boards, plies, layout)
SEARCH = dict(iterations=8, playouts=2, sample_plies=4)


@functools.lru_cache(maxsize=None)
def host_window(boards, plies, layout):
    """Tree-vs-tree self-play of the host flavour with outcome targets, as window_of's arrays (read-only, shared by the tests)."""
    import gobblet_rl_amd as G
    env = G.BatchedGobblet(boards, "cpu", auto_reset=True, seed=boards + plies, track_turn=True)
    traj = env.collect(plies, policies=("tree", "tree"), search=SEARCH, layout=layout, out="fresh")
    env.outcome_targets(traj)
    w = window_of(traj, boards)
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def synthetic_window(n, plies, valid, seed=3):
    """A time-major window of random rows whose valid cells are exactly `valid` (bool (plies, n), row 0 False)."""
    rng = np.random.default_rng(seed)
    stride = -(-n // 64) * 64
    cells = plies * stride
    w = {"obs": rng.integers(0, 2, (cells, 117)).astype(np.int8), "mask": rng.integers(0, 2, (cells, 54)).astype(np.int8),
         "visits": rng.integers(1, 9, (cells, 54)).astype(np.int16), "z": np.full(cells, Z_OPEN, np.int8),
         "done": np.zeros(cells, np.int8), "mover": rng.integers(0, 2, cells).astype(np.int8),
         "n": n, "plies": plies, "ply_stride": stride, "tile_stride": 64}
    t, b = np.nonzero(valid)
    w["z"][cell(t, b, stride, 64)] = rng.choice(np.array([-1, 0, 1], np.int8), len(t))
    assert np.array_equal(valid_cells(w), valid)
    return w
