"""Prioritised replay on the MI355X (-m gpu): the kernels of gbl_replay_prio_append, _update, _index and gbl_replay_batch_prio against the
host flavour bit for bit (which tests/test_replay_prio.py holds to the restatement of the header), every array read back through guard
bytes.  Shapes: rings of one slot, of a ragged second leaf, of more leaves than a wavefront sums at once, and of more leaves than the
scan's workgroup has threads; batches of one row, a tile less one, a tile, a tile and a row, and 65 tiles and a row; windows whose
boards are no multiple of 64 in both layouts, with the cut; updates that all name one slot and that name 4 096 different ones.  The draw
grid and the largest ring run a second time with priorities near 2^31 - 1 (W beyond 2^32, 2^40 and 2^50), and the device index is
compared with the host flavour's in every word.  (Counters and byte offsets past 32 bits: tests/test_gpu_replay_wide.py.)"""
import json
import os

import numpy as np
import pytest
import torch

from tests import replay_prio_restatement as P
from tests import replay_restatement as R
from tests import symmetry_restatement as S
from tests.search_harness import G, replay_arg_errors  # noqa: F401  (G: the fixture)
from tests.test_gpu_replay import DEV, JUNK, DeviceRing, Guarded, device_append, on_device

pytestmark = pytest.mark.gpu

SEED, BASE = 0x1234567890ABCDEF, (1 << 40) + 5
SHAPES = {"obs": (117, np.int8), "mask": (54, np.int8), "visits": (54, np.int16), "z": (None, np.int8), "index": (2, np.int32),
          "sym": (None, np.int16), "prio": (None, np.int32)}


def ring_at(capacity, total, observations=True):
    ring = R.new_ring(capacity, observations, junk=capacity % 1000 + total % 1000)
    ring["meta"][:, R.META_MOVER] &= 1
    ring["state"][0] = total
    return ring


def random_priorities(capacity, total, seed=0):
    """About a third of the rows weightless or negative; garbage where the ring is not live."""
    rng = np.random.default_rng(seed + capacity)
    p = rng.integers(1, 1000, capacity).astype(np.int32)
    p[rng.random(capacity) < 0.2] = 0
    p[rng.random(capacity) < 0.15] *= -1
    live = min(total, capacity)
    p[live:] = rng.integers(-1 << 31, 1 << 31, capacity - live)
    return p


def device_index(lib, ring, prio):
    """gbl_replay_prio_index into an exactly-sized guarded block (no synchronisation)."""
    need = lib.gbl_replay_prio_index_bytes(ring.capacity)
    block = Guarded(np.full(need // 8, 0x5A5A5A5A5A5A5A5A, np.uint64))
    rc = lib.gbl_replay_prio_index(prio.ptr, ring.capacity, ring.ptr("state"), block.ptr, need, None)
    assert rc == 0, lib.gbl_last_error()
    return block


def device_batch(lib, ring, prio, index, batch, sym_mask, call, recent, sync=True):
    keys = [k for k in R.BATCH_OUT + ("prio",) if k != "obs" or "obs" in ring.a]
    out = {k: Guarded(np.full((batch,) if SHAPES[k][0] is None else (batch, SHAPES[k][0]), 77, SHAPES[k][1])) for k in keys}
    out["total"] = Guarded(np.full(2, 7777, np.uint64))
    rc = lib.gbl_replay_batch_prio(ring.ptr("obs"), ring.ptr("visits"), ring.ptr("meta"), ring.capacity, ring.ptr("state"), prio.ptr, index.ptr,
                                   out["prio"].ptr, out["total"].ptr, recent, batch, sym_mask, SEED, BASE, call,
                                   *[out[k].ptr if k in out else None for k in R.BATCH_OUT], None)
    assert rc == 0, lib.gbl_last_error()
    if sync:
        torch.cuda.synchronize()
        return {k: o.read() for k, o in out.items()}
    return out


def host_batch(cpu, host, prio, batch, sym_mask, call, recent, index=None):
    index = P.run_index(cpu, host, prio) if index is None else index
    return P.run_batch(cpu, host, prio, index, batch, sym_mask, SEED, BASE, call, recent)


def draw_grid(G, capacity, priorities, floor=0):
    """Draws of every batch size on a ring not yet wrapped and on a wrapped one, over everything and over a span that reaches back across
    slot 0, and the whole index word for word, device against host flavour; every draw's W is above `floor`."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    for total in sorted({max(2 * capacity // 3, 1), 2 * capacity + capacity // 2 + 1}):   # not yet wrapped (full at one slot), wrapped mid-ring
        host = ring_at(capacity, total)
        prio = priorities(capacity, total)
        if capacity == 1:
            prio[0] = 3
        ring, dprio = DeviceRing(host), Guarded(prio)
        index = device_index(lib, ring, dprio)
        hindex = P.run_index(cpu, host, prio)
        newest = (total - 1) % capacity
        for recent in sorted({0, min(capacity, newest + 3)}):   # everything; a span that reaches back across slot 0 on the wrapped ring
            for batch in (1, 63, 64, 65, 4161):
                got = device_batch(lib, ring, dprio, index, batch, 511, 3, recent)
                P.same_batch(got, host_batch(cpu, host, prio, batch, 511, 3, recent, hindex))
                assert int(got["total"][0]) > floor
        words = index.read()
        assert words[0] == hindex[0] == total and words[1] == hindex[1]
        assert words.dtype == hindex.dtype and np.array_equal(words, hindex), np.argwhere(words != hindex)[:5]   # every word, not only those a draw read
        assert np.array_equal(dprio.read(), prio)
        R.same_ring(ring.read(), host)   # (a draw writes nothing into the ring)


@pytest.mark.parametrize("capacity", [1, 33, 4097])
def test_draw_equals_host_flavour(G, capacity):
    draw_grid(G, capacity, random_priorities)


@pytest.mark.parametrize("capacity,floor", [(33, 1 << 32), (4097, 1 << 40)])
def test_draw_with_weights_beyond_32_bits_equals_host_flavour(G, capacity, floor):
    """The same grid with live priorities within 1 000 of 2^31 - 1 (P.wide_priorities): every W passes 2^32 (2^40 on the larger ring), so
    the upper halves of the index's words, of the sums in its two kernels, of the product in replay_mulhi64 and of both binary searches'
    comparisons are not zero on the device."""
    draw_grid(G, capacity, P.wide_priorities, floor)


def slot_marked_ring(capacity, total):
    """A ring without observations, zeros but for what tells the slots apart (random rows would take seconds to make)."""
    host = R.new_ring(capacity, observations=False)
    slot = np.arange(capacity)
    host["visits"][:, 0], host["visits"][:, 53], host["meta"][:, 7], host["meta"][:, R.META_Z] = slot & 0x7FFF, slot >> 15, slot & 1, slot % 3 - 1
    host["meta"][:, R.META_TAG:R.META_TAG + 4] = slot.astype("<i4").view(np.int8).reshape(-1, 4)
    host["state"][0] = total
    return host


def test_a_ring_of_more_leaves_than_the_scan_has_threads(G):
    """2^21 + 33 slots: 65 538 leaves, so the scan's threads walk stretches of 65 leaves and the last leaf holds one slot; wrapped with the
    newest row mid-ring and `recent` reaching back across slot 0.  A ring without observations (the draw's phase 1 is what is new).  The
    index built twice gives the same draws."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    capacity = (1 << 21) + 33
    total = 3 * capacity + 1000
    host = slot_marked_ring(capacity, total)
    prio = random_priorities(capacity, total)
    ring, dprio = DeviceRing(host), Guarded(prio)
    hindex = P.run_index(cpu, host, prio)
    draws = []
    for _ in range(2):
        index = device_index(lib, ring, dprio)
        got = [device_batch(lib, ring, dprio, index, 4161, 511, 1, recent) for recent in (0, 5000, capacity - 7)]
        draws.append(got)
        words = index.read()
        assert words[0] == total and words[1] == hindex[1] == P.weights(prio).sum()
    for g0, g1, recent in zip(draws[0], draws[1], (0, 5000, capacity - 7)):
        P.same_batch(g0, g1)
        P.same_batch(g0, host_batch(cpu, host, prio, 4161, 511, 1, recent, hindex))
    slots = draws[0][1]["index"][:, 0]
    assert (slots < 1000).any() and (slots >= capacity - 4000).any()   # recent = 5 000 crossed the ring's end
    # not wrapped, the newest row in the ragged last leaf: garbage behind it counts nothing
    host["state"][0] = capacity - 1
    prio[capacity - 1] = (1 << 31) - 1
    ring, dprio = DeviceRing(host), Guarded(prio)
    got = device_batch(lib, ring, dprio, device_index(lib, ring, dprio), 65, 7, 2, 40)
    P.same_batch(got, host_batch(cpu, host, prio, 65, 7, 2, 40))
    assert got["total"][1] == 40 and (got["index"][:, 0] < capacity - 1).all()


def test_the_large_ring_with_weights_beyond_32_bits(G):
    """The ring above (2^21 + 33 slots, wrapped) with P.wide_priorities: W is about 2^51, the blocks' bases pass 2^32 from the second block
    on and a leaf's local prefix from its block's second leaf on.  The whole index and 4 161 draws at three spans against the host flavour;
    prio_out is the weight of the drawn slot."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    capacity = (1 << 21) + 33
    total = 3 * capacity + 1000
    host = slot_marked_ring(capacity, total)
    prio = P.wide_priorities(capacity, total)
    ring, dprio = DeviceRing(host), Guarded(prio)
    hindex = P.run_index(cpu, host, prio)
    index = device_index(lib, ring, dprio)
    for recent in (0, 5000, capacity - 7):
        got = device_batch(lib, ring, dprio, index, 4161, 511, 1, recent)
        P.same_batch(got, host_batch(cpu, host, prio, 4161, 511, 1, recent, hindex))
        drawn = got["index"][:, 0]
        assert (drawn >= 0).all() and np.array_equal(got["prio"], P.weights(prio[drawn]).astype(np.int32)) and (got["prio"] > 0).all()
        assert int(got["total"][0]) > (1 << 50 if recent != 5000 else 1 << 42)
    words = index.read()
    assert words.dtype == hindex.dtype and np.array_equal(words, hindex), np.argwhere(words != hindex)[:5]
    assert int(words[1]) == int(P.weights(prio).sum()) > 1 << 50
    assert np.array_equal(dprio.read(), prio)


def test_failed_samples_without_weight_and_with_a_stale_index(G):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    host = ring_at(200, 450)
    prio = np.where(np.arange(200) % 3 == 0, 0, -5).astype(np.int32)   # W == 0
    ring, dprio = DeviceRing(host), Guarded(prio)
    got = device_batch(lib, ring, dprio, device_index(lib, ring, dprio), 65, 511, 0, 0)
    P.same_batch(got, host_batch(cpu, host, prio, 65, 511, 0, 0))
    assert (got["index"] == -1).all() and got["total"].tolist() == [0, 200] and not got["obs"].any() and (got["z"] == R.Z_OPEN).all()
    empty = ring_at(50, 0)
    ring, dprio = DeviceRing(empty), Guarded(np.full(50, 9, np.int32))
    got = device_batch(lib, ring, dprio, device_index(lib, ring, dprio), 65, 511, 0, 0)
    P.same_batch(got, host_batch(cpu, empty, np.full(50, 9, np.int32), 65, 511, 0, 0))
    assert (got["index"] == -1).all() and got["total"].tolist() == [0, 0]
    # an append after the build: the old index is refused, a new one serves
    w = R.real_window("time")
    host, prio = R.new_ring(300, junk=3), np.full(300, 2, np.int32)
    ring, dprio = DeviceRing(host), Guarded(prio)
    wd = on_device(w)
    device_append(lib, ring, w, wd, 1)
    index = device_index(lib, ring, dprio)
    device_append(lib, ring, w, wd, 2)
    got = device_batch(lib, ring, dprio, index, 65, 511, 0, 0)
    for g in (1, 2):
        R.run_append(cpu, host, w, g)
    P.same_batch(got, host_batch(cpu, host, prio, 65, 511, 0, 0, index.read()))
    assert (got["index"] == -1).all() and got["total"].tolist() == [0, int(host["state"][0])] and not got["prio"].any()
    got = device_batch(lib, ring, dprio, device_index(lib, ring, dprio), 65, 511, 0, 0)
    P.same_batch(got, host_batch(cpu, host, prio, 65, 511, 0, 0))
    assert (got["index"][:, 0] >= 0).all()


def tile_major(w):
    """The time-major window `w` with its cells laid out tile by tile: cell(t, b) = (b // 64) * (64 plies) + 64 t + b % 64."""
    n, plies, tiles = w["n"], w["plies"], -(-w["n"] // 64)
    t, tile, lane = np.meshgrid(np.arange(plies), np.arange(tiles), np.arange(64), indexing="ij")
    src, dst = (t * w["ply_stride"] + tile * 64 + lane).ravel(), (tile * plies * 64 + t * 64 + lane).ravel()
    out = dict(w, ply_stride=64, tile_stride=plies * 64)
    for k, v in w.items():
        if isinstance(v, np.ndarray):
            out[k] = np.empty_like(v)
            out[k][dst] = v[src]
    assert np.array_equal(S.valid_cells(out), S.valid_cells(w))
    return out


def device_prio_append(lib, ring, dprio, w, wd, prio_traj, value):
    rc = lib.gbl_replay_prio_append(wd["visits"].data_ptr(), wd["z"].data_ptr(), wd["done"].data_ptr(),
                                    None if prio_traj is None else prio_traj.data_ptr(), value, w["n"], w["plies"], w["ply_stride"],
                                    w["tile_stride"], dprio.ptr, ring.capacity, ring.ptr("state"), ring.ws.ptr, ring.ws.nbytes, None)
    assert rc == 0, lib.gbl_last_error()


@pytest.mark.parametrize("layout", ["time", "tile"])
@pytest.mark.parametrize("boards,plies", [(65, 3), (257, 5)])
def test_prio_append_equals_host_flavour(G, layout, boards, plies):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    valid = np.random.default_rng(boards).random((plies, boards)) < 0.6
    valid[0] = False
    w = S.synthetic_window(boards, plies, valid, seed=plies)
    if layout == "tile":
        w = tile_major(w)
    assert (w["tile_stride"] == 64) == (layout == "time")
    K = int(valid.sum())
    wd = on_device(w)
    per_cell = np.random.default_rng(6).integers(-50, 1000, w["z"].shape[0]).astype(np.int32)
    per_cell_dev = torch.from_numpy(per_cell).to(DEV)
    for capacity in (K + 9, K - 1, K // 2, 1):   # larger than the window, the cut of one row, of half the rows, one slot
        for prio_traj, dev_traj, value in ((None, None, 6), (per_cell, per_cell_dev, 0)):
            host, prio = R.new_ring(capacity, observations=False, junk=2), np.full(capacity, P.FILL, np.int32)
            ring, dprio = DeviceRing(host), Guarded(prio)
            for g in range(2):   # (the second append wraps)
                device_append(lib, ring, w, wd, g)
                device_prio_append(lib, ring, dprio, w, wd, dev_traj, value + g)   # on the same stream, nothing in between
                R.run_append(cpu, host, w, g)
                P.run_prio_append(cpu, host, prio, w, prio_traj, value + g)
            torch.cuda.synchronize()
            ring.ws.read()
            assert np.array_equal(dprio.read(), prio), (capacity, value)
            R.same_ring(ring.read(), host)
            assert capacity < 2 * K or (prio == P.FILL).sum() == capacity - 2 * K


def test_prio_update_under_contention_and_with_distinct_slots(G):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    rng = np.random.default_rng(2)
    capacity, batch = 5000, 4096
    values = rng.integers(-1000, 1000, batch).astype(np.int32)
    cases = {"one slot": np.full(batch, 4321), "distinct": rng.permutation(capacity)[:batch],
             "mixed": np.concatenate([rng.integers(-3, capacity + 3, batch - 100), np.full(100, -1)])}
    for name, slots in cases.items():
        index = np.stack([slots, rng.integers(0, 9, batch)], 1).astype(np.int32)
        prio = rng.integers(2000, 3000, capacity).astype(np.int32)   # (above every value: the old priority must not survive)
        dprio, dindex, dvalues = Guarded(prio), torch.from_numpy(index).to(DEV), torch.from_numpy(values).to(DEV)
        rc = lib.gbl_replay_prio_update(dindex.data_ptr(), dvalues.data_ptr(), batch, dprio.ptr, capacity, None)
        assert rc == 0, lib.gbl_last_error()
        torch.cuda.synchronize()
        P.run_prio_update(cpu, prio, index, values)
        assert np.array_equal(dprio.read(), prio), name
        if name == "one slot":
            assert prio[4321] == values.max() and (prio != values.max()).sum() == capacity - 1
    assert lib.gbl_replay_prio_update(None, None, 0, None, capacity, None) == 0


def test_append_prio_append_index_and_draw_in_stream_order(G):
    """The four on one stream with no synchronisation in between: the draw sees the appended rows, their priorities and the new index."""
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    w = R.real_window("time")
    wd = on_device(w)
    per_cell = (np.arange(w["z"].shape[0]) % 11).astype(np.int32)
    per_cell_dev = torch.from_numpy(per_cell).to(DEV)
    host, prio = R.new_ring(100, junk=6), np.zeros(100, np.int32)
    ring, dprio = DeviceRing(host), Guarded(prio)
    torch.cuda.synchronize()
    device_append(lib, ring, w, wd, 21)
    device_prio_append(lib, ring, dprio, w, wd, per_cell_dev, 0)
    index = device_index(lib, ring, dprio)
    out = device_batch(lib, ring, dprio, index, 200, 511, 1, 0, sync=False)
    torch.cuda.synchronize()
    R.run_append(cpu, host, w, 21)
    P.run_prio_append(cpu, host, prio, w, per_cell, 0)
    P.same_batch({k: o.read() for k, o in out.items()}, host_batch(cpu, host, prio, 200, 511, 1, 0))
    assert np.array_equal(dprio.read(), prio)
    R.same_ring(ring.read(), host)


def test_prioritized_buffer_fits_alike_on_either_device(G):
    """Through the binding: the same self-play window appended twice with per-cell priorities to a ReplayBuffer on cuda:0 and on cpu, rows
    re-prioritised from a draw, 3 steps of a prioritised fit at H = 64."""
    fits = []
    for d in (DEV, "cpu"):
        env = G.BatchedGobblet(130, d, auto_reset=True, seed=5, track_turn=True)
        traj = env.collect(6, policies=("tree", "tree"), search=S.SEARCH)
        env.outcome_targets(traj)
        buf = G.ReplayBuffer(150, d, prioritized=True)
        cells = (torch.arange(traj["z"].numel(), device=d).reshape(traj["z"].shape) % 7).to(torch.int32)
        buf.append(env, traj, tag=1, priority=3)
        buf.append(env, traj, tag=2, priority=cells)
        first = buf.batch(300, call=1, seed=4, prioritized=True)
        buf.set_priority(first["index"], (first["priority"] + first["sym"].to(torch.int32)) % 9)
        trainer = G.GobbletTrainer(hidden=64, device=d, seed=1)
        fits.append((buf, trainer, buf.fit(trainer, 3, batch=256, recent=120, prioritized=True), first,
                     G.ReplayBuffer.importance_weights(buf.batch(64, call=9, prioritized=True), 0.5)))
    (gb, gt, gs, gf, gw), (cb, ct, cs, cf, cw) = fits
    assert gb.total == cb.total > 150 and torch.equal(gb.priority.cpu(), cb.priority) and len(set(cb.priority.tolist())) > 5
    assert all(torch.equal(gf[k].cpu(), cf[k]) for k in cf) and set(cf) >= {"priority", "prio_total"}
    assert torch.equal(gs.cpu(), cs) and float(cs[:, 2].min()) == 256
    assert torch.equal(gt.params.cpu(), ct.params) and torch.equal(gt.v.cpu(), ct.v)
    assert torch.allclose(gw.cpu(), cw, rtol=1e-6, atol=0) and float(cw.max()) == 1.0   # (torch's pow, not the library's: no bit rule)


def test_argument_errors_replay_the_recorded_table(G, golden_dir):
    replay_arg_errors(json.load(open(os.path.join(golden_dir, "replay_prio_arg_errors.json"))), flavours=("device",))
    torch.cuda.synchronize()
