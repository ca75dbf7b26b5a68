"""The "Replay buffer" paragraph of include/gobblet_hip.h restated in numpy from the header's text: the ring's three arrays and its
state, the append rule (valid cells in ascending (t, b), slot (T0 + r) mod capacity, the K - capacity cut, zero padding) and the draw
rule of gbl_replay_batch (one Philox block on stream 7, age, slot, symmetry).  The valid cells, the symmetries and the generator come
from tests/symmetry_restatement.py and the oracle; no code or table shared with the library (test infrastructure).  Also the rings and
the calls through a library handle that the CPU and the GPU tests share."""
import functools

import numpy as np

import oracle

from tests import symmetry_restatement as S

OBS_PITCH, VISITS_PITCH, META_PITCH = 128, 64, 64   # GBL_REPLAY_*_PITCH
META_Z, META_MOVER, META_TAG = 54, 55, 56
STREAM, Z_OPEN = 7, -128
BATCH_OUT = S.BATCH_OUT


def new_ring(capacity, observations=True, junk=None):
    """A fresh ring (all zeros), or with `junk` one whose every byte is junk (a seed): what an append must leave alone."""
    rng = None if junk is None else np.random.default_rng(junk)
    fill = (lambda shape, dt: np.zeros(shape, dt)) if rng is None else \
        (lambda shape, dt: rng.integers(np.iinfo(dt).min, np.iinfo(dt).max + 1, shape).astype(dt))
    return {"obs": fill((capacity, OBS_PITCH), np.int8) if observations else None, "visits": fill((capacity, VISITS_PITCH), np.int16),
            "meta": fill((capacity, META_PITCH), np.int8), "state": np.zeros(2, np.uint64), "capacity": capacity}


def copy_ring(ring):
    return {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in ring.items()}


def same_ring(got, exp):
    for k in ("obs", "visits", "meta", "state"):
        if exp[k] is None:
            assert got[k] is None
            continue
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (k, np.argwhere(got[k] != exp[k])[:5])


def append(ring, w, tag):
    """gbl_replay_append by the header's rule, in place; returns K."""
    t, b = np.nonzero(S.valid_cells(w))   # (row-major: ascending (t, b), t outer)
    K, cap, T0 = len(t), ring["capacity"], int(ring["state"][0])
    r = np.arange(K, dtype=np.int64)
    keep = r >= K - cap
    slots = np.array([(T0 + int(i)) % cap for i in r[keep]], np.int64)
    assert len(set(slots.tolist())) == len(slots)
    at = S.cell(t[keep], b[keep], w["ply_stride"], w["tile_stride"])
    prev = S.cell(t[keep] - 1, b[keep], w["ply_stride"], w["tile_stride"])
    if ring["obs"] is not None:
        rows = np.zeros((len(slots), OBS_PITCH), np.int8)
        rows[:, :117] = w["obs"][prev]
        ring["obs"][slots] = rows
    rows = np.zeros((len(slots), VISITS_PITCH), np.int16)
    rows[:, :54] = w["visits"][at]
    ring["visits"][slots] = rows
    rows = np.zeros((len(slots), META_PITCH), np.int8)
    rows[:, :54] = w["mask"][prev]
    rows[:, META_Z] = w["z"][at]
    rows[:, META_MOVER] = w["mover"][at] != 0
    rows[:, META_TAG:META_TAG + 4] = np.array([tag], "<i4").view(np.int8)
    ring["meta"][slots] = rows
    ring["state"][:] = T0 + K, K
    return K


def batch(ring, batch, sym_mask, seed, sample_base, call, recent):
    """The outputs of gbl_replay_batch by the header's rule, as a dict over BATCH_OUT."""
    cap, total = ring["capacity"], int(ring["state"][0])
    live = min(total, cap)
    key = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]
    out = {"obs": np.zeros((batch, 117), np.int8), "mask": np.zeros((batch, 54), np.int8), "visits": np.zeros((batch, 54), np.int16),
           "z": np.full(batch, Z_OPEN, np.int8), "index": np.full((batch, 2), -1, np.int32), "sym": np.zeros(batch, np.int16)}
    if ring["obs"] is None:
        del out["obs"]
    if live == 0:
        return out
    span = min(recent, live) if recent > 0 else live
    slot, s = np.zeros(batch, np.int64), np.zeros(batch, np.int64)
    for j in range(batch):
        ident = sample_base + j
        w0, _, w2, _ = (int(x) for x in oracle.philox4x32_10([ident & 0xFFFFFFFF, (ident >> 32) & 0xFFFFFFFF, 16 * call, STREAM], key))
        age = (w0 * span) >> 32
        slot[j], s[j] = (total - 1 - age) % cap, w2 & sym_mask
    meta = ring["meta"][slot]
    rows = dict(mask=meta[:, :54], visits=ring["visits"][slot][:, :54])
    if ring["obs"] is not None:
        rows["obs"] = ring["obs"][slot][:, :117]
    out.update(S.apply(s, meta[:, META_MOVER], **rows))
    out["z"], out["sym"] = meta[:, META_Z].copy(), s.astype(np.int16)
    out["index"] = np.stack([slot, np.ascontiguousarray(meta[:, META_TAG:META_TAG + 4]).view("<i4")[:, 0]], 1).astype(np.int32)
    return out


def workspace_bytes(n, plies):
    """32 + 16 per chunk, (plies - 1) * ceil(n / 64) chunks."""
    return 32 + 16 * (plies - 1) * -(-n // 64)


def run_append(lib, ring, w, tag, prefix="gbl_cpu_"):
    """gbl_replay_append on a numpy ring through a raw handle, in place (the workspace pre-filled with junk)."""
    need = workspace_bytes(w["n"], w["plies"])
    ws = np.full(need, 0x5A, np.uint8)
    obs = ring["obs"] is not None
    rc = getattr(lib, prefix + "replay_append")(
        w["obs"].ctypes.data if obs else None, *[w[k].ctypes.data for k in ("mask", "visits", "z", "done", "mover")], w["n"], w["plies"],
        w["ply_stride"], w["tile_stride"], tag, ring["obs"].ctypes.data if obs else None, ring["visits"].ctypes.data, ring["meta"].ctypes.data,
        ring["capacity"], ring["state"].ctypes.data, ws.ctypes.data, need, None)
    assert rc == 0, getattr(lib, prefix + "last_error")()


def run_batch(lib, ring, batch, sym_mask, seed, sample_base, call, recent, prefix="gbl_cpu_"):
    """gbl_replay_batch on a numpy ring through a raw handle: dict over BATCH_OUT (without "obs" for a ring without), pre-filled with junk."""
    out = {"obs": np.full((batch, 117), 77, np.int8), "mask": np.full((batch, 54), 77, np.int8), "visits": np.full((batch, 54), 7777, np.int16),
           "z": np.full(batch, 77, np.int8), "index": np.full((batch, 2), 7777, np.int32), "sym": np.full(batch, 7777, np.int16)}
    if ring["obs"] is None:
        del out["obs"]
    rc = getattr(lib, prefix + "replay_batch")(
        None if ring["obs"] is None else ring["obs"].ctypes.data, ring["visits"].ctypes.data, ring["meta"].ctypes.data, ring["capacity"],
        ring["state"].ctypes.data, recent, batch, sym_mask, seed, sample_base, call,
        *[out[k].ctypes.data if k in out else None for k in BATCH_OUT], None)
    assert rc == 0, getattr(lib, prefix + "last_error")()
    return out


def same_batch(got, exp, batch=None):
    assert set(got) == set(exp)
    for k in got:
        g, e = (got[k], exp[k]) if batch is None else (got[k][:batch], exp[k][:batch])
        assert g.dtype == e.dtype and np.array_equal(g, e), (k, np.argwhere(g != e)[:5])


# ---- the windows ---------------------------------------------------------------------------------------------------------------------
REAL = (130, 6)   # boards, plies: tree-vs-tree self-play of the host flavour, 8 iterations and 2 playouts (S.SEARCH), outcome targets


def real_window(layout):
    return S.host_window(*REAL, layout)


@functools.lru_cache(maxsize=None)
def synthetic(kind, n=130, plies=5):
    """A time-major window of random rows: every cell valid, no cell valid, or a checkerboard over (t, b)."""
    valid = np.zeros((plies, n), bool)
    if kind == "all":
        valid[1:] = True
    elif kind == "checkerboard":
        t, b = np.meshgrid(np.arange(plies), np.arange(n), indexing="ij")
        valid = ((t + b) % 2 == 0) & (t > 0)
    else:
        assert kind == "none"
    w = S.synthetic_window(n, plies, valid, seed=plies + n)
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return w


def count_valid(w):
    return int(S.valid_cells(w).sum())
