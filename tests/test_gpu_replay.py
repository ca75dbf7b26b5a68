"""gbl_replay_append and gbl_replay_batch on the MI355X (-m gpu): the kernels against the host flavour bit for bit (which
tests/test_replay.py holds to the restatement of the header), the ring, its state, the workspace and every output read back through
guard bytes.  Shapes: boards that are no multiple of 64 throughout, both trajectory layouts, rings larger than a window, smaller than
one chunk's rows and of one slot, appends that wrap, more chunks than the scan's workgroup has threads, batches of one row, of a tile,
of a tile and a row, of several tiles with a ragged tail.  (`call` travels by value only, so there is no captured-graph case here.)"""
import json
import os

import numpy as np
import pytest
import torch

from tests import replay_restatement as R
from tests import symmetry_restatement as S
from tests.search_harness import G, replay_arg_errors  # noqa: F401  (G: the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, JUNK = 128, 0x5A   # (a whole line on either side: the payload keeps the ring's 128-byte alignment)
SCAN_THREADS = 1024       # k_replay_scan's workgroup


class Guarded:
    """A device array holding `a` (numpy) with GUARD junk bytes on both sides; the payload starts on a 128-byte line."""

    def __init__(self, a):
        self.shape, self.dtype, self.nbytes = a.shape, a.dtype, a.nbytes
        image = np.concatenate([np.full(GUARD, JUNK, np.uint8), np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.full(GUARD, JUNK, np.uint8)])
        self.raw = torch.from_numpy(image).to(DEV)
        assert self.ptr % 128 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def read(self):
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == JUNK).all() and (raw[GUARD + self.nbytes:] == JUNK).all(), "a guard byte was written"
        return raw[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape)


class DeviceRing:
    """The arrays of a numpy ring on the device, each between guards."""

    def __init__(self, ring):
        self.capacity = ring["capacity"]
        self.a = {k: Guarded(ring[k]) for k in ("obs", "visits", "meta", "state") if ring[k] is not None}

    def ptr(self, k):
        return self.a[k].ptr if k in self.a else None

    def read(self):
        return {"obs": None, **{k: g.read() for k, g in self.a.items()}, "capacity": self.capacity}


def on_device(w):
    return {k: torch.from_numpy(v.copy()).to(DEV) for k, v in w.items() if isinstance(v, np.ndarray)}   # (the shared windows are read-only)


def device_append(lib, ring, w, wd, tag):
    """gbl_replay_append on the device ring (no synchronisation); the workspace is checked when the ring is read."""
    need = lib.gbl_replay_workspace_bytes(w["n"], w["plies"])
    ring.ws = Guarded(np.full(need, JUNK, np.uint8))
    obs = "obs" in ring.a
    rc = lib.gbl_replay_append(wd["obs"].data_ptr() if obs else None, *[wd[k].data_ptr() for k in ("mask", "visits", "z", "done", "mover")],
                               w["n"], w["plies"], w["ply_stride"], w["tile_stride"], tag, ring.ptr("obs"), ring.ptr("visits"), ring.ptr("meta"),
                               ring.capacity, ring.ptr("state"), ring.ws.ptr, need, None)
    assert rc == 0, lib.gbl_last_error()


def device_batch(lib, ring, batch, sym_mask, seed, sample_base, call, recent, only=None, sync=True):
    shapes = {"obs": ((batch, 117), np.int8), "mask": ((batch, 54), np.int8), "visits": ((batch, 54), np.int16), "z": ((batch,), np.int8),
              "index": ((batch, 2), np.int32), "sym": ((batch,), np.int16)}
    keys = [k for k in R.BATCH_OUT if (k != "obs" or "obs" in ring.a) and (only is None or k in only)]
    out = {k: Guarded(np.full(shapes[k][0], 77, shapes[k][1])) for k in keys}
    rc = lib.gbl_replay_batch(ring.ptr("obs"), ring.ptr("visits"), ring.ptr("meta"), ring.capacity, ring.ptr("state"), recent, batch, sym_mask,
                              seed, sample_base, call, *[out[k].ptr if k in out else None for k in R.BATCH_OUT], None)
    assert rc == 0, lib.gbl_last_error()
    if sync:
        torch.cuda.synchronize()
        return {k: o.read() for k, o in out.items()}
    return out


def appended(lib, cpu, capacity, windows, observations=True, junk=1):
    """The windows appended one after the other to a junk-filled ring on the device and on the host: (device ring, host ring)."""
    host = R.new_ring(capacity, observations, junk=junk)
    ring = DeviceRing(host)
    for g, w in enumerate(windows):
        device_append(lib, ring, w, on_device(w), 10 + g)
        torch.cuda.synchronize()
        ring.ws.read()   # (its guards)
        R.run_append(cpu, host, w, 10 + g)
    return ring, host


@pytest.mark.parametrize("layout", ["time", "tile"])
@pytest.mark.parametrize("capacity", [1000, 37, 1])
def test_append_equals_host_flavour(G, layout, capacity):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    w = R.real_window(layout)
    assert w["n"] % 64 and R.count_valid(w) > 64 > 37
    for observations in (True, False):
        ring, host = appended(lib, cpu, capacity, [w], observations)
        R.same_ring(ring.read(), host)


def test_two_appends_that_wrap(G):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    ws = [R.real_window("time"), R.real_window("tile")]
    K = R.count_valid(ws[0])
    ring, host = appended(lib, cpu, K + K // 2, ws)
    assert host["state"].tolist() == [2 * K, K]
    R.same_ring(ring.read(), host)


@pytest.mark.parametrize("capacity", [40000, 20000])
def test_more_chunks_than_the_scan_has_threads(G, capacity):
    """2 100 boards x 33 plies: 32 x 33 = 1 056 chunks, so the scan's threads walk stretches of two chunks (and the last ones none); about
    half the cells valid, at random; the smaller ring is overflowed by the window alone."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    n, plies = 2100, 33
    assert (plies - 1) * -(-n // 64) > SCAN_THREADS and n % 64
    valid = np.random.default_rng(8).random((plies, n)) < 0.5
    valid[0] = False
    w = S.synthetic_window(n, plies, valid, seed=4)
    K = int(valid.sum())
    assert 20000 < K < 40000
    ring, host = appended(lib, cpu, capacity, [w])
    assert host["state"].tolist() == [K, K]
    R.same_ring(ring.read(), host)


@pytest.mark.parametrize("batch", [1, 64, 65, 200])
def test_batch_equals_host_flavour(G, batch):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    ring, host = appended(lib, cpu, 200, [R.real_window("time"), R.real_window("tile")])
    bare, bare_host = appended(lib, cpu, 1000, [R.real_window("time")], observations=False)
    seed, base = 0x1234567890ABCDEF, (1 << 40) + 5
    for sym_mask in (0, 511):
        for recent in (0, 5):
            got, exp = device_batch(lib, ring, batch, sym_mask, seed, base, 3, recent), R.run_batch(cpu, host, batch, sym_mask, seed, base, 3, recent)
            R.same_batch(got, exp)
            R.same_batch(device_batch(lib, bare, batch, sym_mask, seed, base, 3, recent), R.run_batch(cpu, bare_host, batch, sym_mask, seed, base, 3, recent))
    got = device_batch(lib, ring, batch, 511, seed, base, 3, 0, only=("visits", "index"))   # the other outputs NULL
    exp = R.run_batch(cpu, host, batch, 511, seed, base, 3, 0)
    assert set(got) == {"visits", "index"} and np.array_equal(got["visits"], exp["visits"]) and np.array_equal(got["index"], exp["index"])
    R.same_ring(ring.read(), host)   # (a draw writes nothing into the ring)


def test_batch_of_an_empty_buffer(G):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    host = R.new_ring(50, junk=2)
    got = device_batch(lib, DeviceRing(host), 65, 511, 1, 0, 0, 0)
    R.same_batch(got, R.run_batch(cpu, host, 65, 511, 1, 0, 0, 0))
    assert (got["index"] == -1).all() and (got["z"] == R.Z_OPEN).all() and not got["obs"].any()


def test_append_then_batch_in_stream_order(G):
    """Append and draw on one stream with no synchronisation in between: the draw sees the appended rows and the new state."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    w = R.real_window("time")
    wd = on_device(w)
    host = R.new_ring(100, junk=6)
    ring = DeviceRing(host)
    torch.cuda.synchronize()
    device_append(lib, ring, w, wd, 21)
    out = device_batch(lib, ring, 200, 511, 5, 0, 1, 0, sync=False)
    torch.cuda.synchronize()
    R.run_append(cpu, host, w, 21)
    R.same_batch({k: o.read() for k, o in out.items()}, R.run_batch(cpu, host, 200, 511, 5, 0, 1, 0))
    R.same_ring(ring.read(), host)


def test_replay_buffer_fits_alike_on_either_device(G):
    """Through the binding: the same self-play window appended twice to a ReplayBuffer on cuda:0 and on cpu, 3 steps of fit at H = 64."""
    fits = []
    for d in (DEV, "cpu"):
        env = G.BatchedGobblet(130, d, auto_reset=True, seed=5, track_turn=True)
        traj = env.collect(6, policies=("tree", "tree"), search=S.SEARCH)
        env.outcome_targets(traj)
        buf = G.ReplayBuffer(150, d)
        buf.append(env, traj, tag=1)
        buf.append(env, traj, tag=2)
        trainer = G.GobbletTrainer(hidden=64, device=d, seed=1)
        fits.append((buf, trainer, buf.fit(trainer, 3, batch=256, recent=120)))
    (gb, gt, gs), (cb, ct, cs) = fits
    assert gb.total == cb.total > 150 and gb.size == 150
    for name in ("observation", "action_mask", "visits", "z", "mover", "tag"):
        assert torch.equal(getattr(gb, name).cpu(), getattr(cb, name)), name
    assert torch.equal(gs.cpu(), cs) and float(cs[:, 2].min()) == 256
    assert torch.equal(gt.params.cpu(), ct.params) and torch.equal(gt.v.cpu(), ct.v)


def test_argument_errors_replay_the_recorded_table(G, golden_dir):
    replay_arg_errors(json.load(open(os.path.join(golden_dir, "replay_arg_errors.json"))), flavours=("device",))
    torch.cuda.synchronize()
