"""Prioritised replay, host flavour (no GPU): gbl_cpu_replay_prio_append, _update, _index and gbl_cpu_replay_batch_prio against the numpy
restatement of the header's paragraph (tests/replay_prio_restatement.py), bit for bit and every output; the frequencies of the draw on a
small ring; draws of a ring that has taken more than 2^32 rows, the index word for word against its layout, and a ring far along against
a small ring translated (what the device tests past 32 bits rest on); ReplayBuffer(prioritized=True) on the host flavour (the stale-index
bookkeeping, importance weights, fit against the hand-written loop, state_dict; an unprioritised buffer as before) and the recorded
argument errors of both flavours."""
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import replay_prio_restatement as P
from tests import replay_restatement as R
from tests import symmetry_restatement as S
from tests.search_harness import replay_arg_errors

SEED, BASE = 0x1234567890ABCDEF, (1 << 40) + 5
FREQUENCY_SEED = 1   # (the first seed tried: the restatement alone keeps every count within 5 standard deviations, checked below)


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


def ring_at(capacity, total, observations=True):
    """A ring of random rows (mover bytes 0 / 1) that has taken `total` rows."""
    ring = R.new_ring(capacity, observations, junk=capacity + total)
    ring["meta"][:, R.META_MOVER] &= 1
    ring["state"][0] = total
    return ring


def states(capacity):
    """total: not yet wrapped, exactly full, wrapped with the newest row mid-ring"""
    return sorted({max(2 * capacity // 3, 0), capacity, 2 * capacity + capacity // 2 + 1})


def recents(capacity, total):
    live, newest = min(total, capacity), (total - 1) % capacity if total else 0
    return sorted({0, 1, 32, min(live, newest + 3), live + 10})   # (newest + 3 rows reach back across slot 0 on a wrapped ring)


PATTERNS = ("equal", "zero", "one", "interleaved", "negative", "garbage")


def priorities(pattern, capacity, total):
    rng = np.random.default_rng(capacity * 7 + total)
    live = min(total, capacity)
    p = rng.integers(1, 1000, capacity).astype(np.int32)
    if pattern == "equal":
        p[:] = 5
    elif pattern == "zero":
        p[:] = 0
    elif pattern == "one":
        p[:] = 0
        p[rng.integers(0, max(live, 1))] = 9
    elif pattern == "interleaved":
        p[::2] = 0
    elif pattern == "negative":
        p[rng.random(capacity) < 0.5] *= -1
    if pattern == "garbage" or live < capacity:
        p[live:] = rng.integers(-1 << 31, 1 << 31, capacity - live)   # (slots that are not live count 0 whatever they hold)
    return p


def draw_both(cpu, ring, prio, batch, sym_mask, call, recent, sizes=()):
    index = P.run_index(cpu, ring, prio)
    assert int(index[0]) == int(ring["state"][0])
    live = min(int(ring["state"][0]), ring["capacity"])
    assert int(index[1]) == int(P.weights(prio[:live]).sum())
    exp = P.batch(ring, prio, False, batch, sym_mask, SEED, BASE, call, recent)
    P.same_batch(P.run_batch(cpu, ring, prio, index, batch, sym_mask, SEED, BASE, call, recent), exp)
    for n in sizes:   # a batch is the beginning of every longer one
        P.same_batch(P.run_batch(cpu, ring, prio, index, n, sym_mask, SEED, BASE, call, recent), exp, n)
    return exp, index


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [1, 31, 32, 33, 1000])
def test_draw_host_flavour_equals_restatement(cpu, capacity):
    seen = set()
    for total in states(capacity):
        ring = ring_at(capacity, total)
        live = min(total, capacity)
        for pattern in PATTERNS:
            prio = priorities(pattern, capacity, total)
            w = P.weights(prio)
            for recent in recents(capacity, total):
                exp, _ = draw_both(cpu, ring, prio, 65, 511, 3, recent, sizes=(0, 1, 63, 64) if recent in (0, 32) else ())
                span = min(recent, live) if recent > 0 else live
                slots = [(total - span + q) % capacity for q in range(span)]
                W = int(w[slots].sum()) if span else 0
                assert exp["total"].tolist() == [W, span]
                if W == 0:
                    assert (exp["index"] == -1).all() and (exp["z"] == R.Z_OPEN).all() and not exp["prio"].any() and not exp["obs"].any()
                    seen.add("failed")
                    continue
                drawn = exp["index"][:, 0]
                assert set(drawn.tolist()) <= set(slots) and (w[drawn] > 0).all() and np.array_equal(exp["prio"], w[drawn])
                if pattern == "one" and W == 9:
                    assert len(set(drawn.tolist())) == 1
                    seen.add("one")
                if slots and slots[0] > slots[-1]:
                    seen.add("crossing")
    assert {"failed", "one"} <= seen and (capacity == 1 or "crossing" in seen)


def test_weights_beyond_32_bits(cpu):
    """4 096 rows near 2^31 - 1: W > 2^32, the high half of the 64 x 64 product matters in every bit."""
    capacity, total = 5000, 4096 + 5000
    ring, rng = ring_at(capacity, total, observations=False), np.random.default_rng(3)
    prio = np.zeros(capacity, np.int32)
    prio[rng.choice(capacity, 4096, replace=False)] = (1 << 31) - 1 - rng.integers(0, 1000, 4096)
    for recent in (0, 4500):
        exp, _ = draw_both(cpu, ring, prio, 300, 7, 1, recent)
        assert int(exp["total"][0]) > 1 << 42 and len(set(exp["index"][:, 0].tolist())) > 250 and (exp["prio"] > (1 << 31) - 1002).all()


@pytest.mark.parametrize("capacity", [33, 1000])
def test_draw_of_a_ring_that_has_taken_more_than_2_to_the_32_rows(cpu, capacity):
    """state[0] beyond 2^32 (the span's first slot is (total - span) mod capacity in 64 bits) with weights near 2^31 - 1, about 30 % of
    them 0: W passes 2^32, so r = floor(u W / 2^64) needs every one of the four partial products.  `recent` = 7 and capacity - 1: prefixes
    that end inside a leaf, one span that crosses slot 0."""
    crossed = False
    for total in ((1 << 32) + 5, 3 * (1 << 32) + capacity // 2, (1 << 40) + 3):
        ring = ring_at(capacity, total)
        rng = np.random.default_rng(capacity + total % 1000)
        prio = ((1 << 31) - 1 - rng.integers(0, 1000, capacity)).astype(np.int32)
        prio[rng.random(capacity) < 0.3] = 0
        for recent in (0, 7, capacity - 1):
            exp, _ = draw_both(cpu, ring, prio, 65, 511, 3, recent)
            span = recent if recent else capacity
            slots = [(total - span + q) % capacity for q in range(span)]
            assert total % capacity != (total & 0xFFFFFFFF) % capacity
            W = int(P.weights(prio[slots]).sum())
            assert exp["total"].tolist() == [W, span] and (W > 1 << 32 or recent == 7)
            drawn = exp["index"][:, 0]
            assert set(drawn.tolist()) <= set(slots) and np.array_equal(exp["prio"], prio[drawn]) and (exp["prio"] > 0).all()
            crossed |= slots[0] > slots[-1]
    assert crossed


def test_a_ring_far_along_is_a_small_ring_translated(cpu):
    """What tests/test_gpu_replay_wide.py rests on, here on the host flavour: a window of K rows appended at state[0] = T0 >= 2^33 leaves in
    slot (T0 + r) mod capacity what it leaves in slot r of a ring of exactly K slots appended at 0 -- rows and priorities --, the uniform
    draw over the newest K rows and the weighted draws (every other priority 0) are the small ring's with the slots translated.  Mid-ring
    and across the ring's end."""
    w = R.real_window("time")
    K, capacity = R.count_valid(w), 1097
    rng = np.random.default_rng(7)
    per_cell = ((1 << 31) - 1 - rng.integers(0, 1000, w["z"].shape[0])).astype(np.int32)
    per_cell[rng.random(len(per_cell)) < 0.25] = 0
    small, sprio = R.new_ring(K), np.zeros(K, np.int32)
    R.run_append(cpu, small, w, 9)
    P.run_prio_append(cpu, small, sprio, w, per_cell, 0)
    sindex = P.run_index(cpu, small, sprio)
    for m, first in (((1 << 33) // capacity + 1, 400), ((1 << 52) // capacity + 3, capacity - K // 2)):
        T0 = m * capacity + first
        assert T0 >= 1 << 33 and T0 % capacity == first and T0 % capacity != (T0 & 0xFFFFFFFF) % capacity
        ring, prio = R.new_ring(capacity), np.zeros(capacity, np.int32)
        ring["state"][0] = T0
        R.run_append(cpu, ring, w, 9)
        P.run_prio_append(cpu, ring, prio, w, per_cell, 0)
        slots = (T0 + np.arange(K)) % capacity
        assert ring["state"].tolist() == [T0 + K, K] and np.array_equal(prio[slots], sprio) and np.count_nonzero(prio) == np.count_nonzero(sprio)
        for k in ("obs", "visits", "meta"):
            assert np.array_equal(ring[k][slots], small[k]) and np.count_nonzero(ring[k]) == np.count_nonzero(small[k]), k
        index = P.run_index(cpu, ring, prio)
        exp = R.run_batch(cpu, small, 130, 511, SEED, BASE, 3, 0)
        exp["index"][:, 0] = (T0 + exp["index"][:, 0].astype(np.int64)) % capacity
        R.same_batch(R.run_batch(cpu, ring, 130, 511, SEED, BASE, 3, K), exp)
        exp = P.run_batch(cpu, small, sprio, sindex, 130, 511, SEED, BASE, 3, 0)
        exp["index"][:, 0] = (T0 + exp["index"][:, 0].astype(np.int64)) % capacity
        for recent in (0, K, K + 50):
            exp["total"][1] = recent if recent else capacity
            P.same_batch(P.run_batch(cpu, ring, prio, index, 130, 511, SEED, BASE, 3, recent), exp)


@pytest.mark.parametrize("capacity", [1, 33, 4097, (1 << 27) + 3 * 2048 + 33])
def test_index_of_the_host_flavour_word_for_word(cpu, capacity):
    """Every word of the host flavour's index against P.index_layout: the layout that the two flavours share (csrc/gobblet_cpu.cpp builds
    the device flavour's, csrc/gobblet_device.h states it), NOT the ABI -- the header keeps the index opaque, and only the library reads
    it.  The device tests compare the kernels' index with this one word for word, so this closes the chain for the words no draw happens
    to read.  The last capacity has more blocks than the leaves kernel has workgroups and a ragged last leaf of one slot; W is about
    2^57.5 there.  At that size the states are those of the device test (tests/test_gpu_replay_wide.py): wrapped, and capacity - 1 and
    capacity - 3 with the LARGEST weight in every slot that is not live, so an index that counted one of them differs."""
    big = capacity > 1 << 27
    totals = (3 * capacity + 1000, capacity - 1, capacity - 3) if big else (3 * capacity + 1000, max(2 * capacity // 3, 1))
    prio = None
    for total in totals:   # wrapped; not wrapped, garbage behind the live rows
        if big and prio is not None:   # (one array at this size: making it is what costs)
            prio[total:] = (1 << 31) - 1
            assert (prio[capacity - 5:] > 0).all()   # live and dead entries of the last vectors alike
        else:
            prio = P.wide_priorities(capacity, total)
        if capacity == 1:
            prio[0] = (1 << 31) - 1
        ring = {"capacity": capacity, "state": np.array([total, 0], np.uint64)}
        got = P.run_index(cpu, ring, prio)
        exp = P.index_layout(prio, capacity, total)
        assert got.dtype == exp.dtype and np.array_equal(got, exp), np.argwhere(got != exp)[:5]
        assert int(got[1]) == int(np.maximum(prio[:min(total, capacity)], 0).sum(dtype=np.int64)) > 0
        if big:
            assert int(got[1]) > 1 << 57 and len(got) == 2 + 65540 + 1 + 4194498


def test_every_optional_output_null_in_turn_and_a_ring_without_observations(cpu):
    ring = ring_at(200, 450)
    prio = priorities("interleaved", 200, 450)
    exp, index = draw_both(cpu, ring, prio, 130, 511, 2, 0)
    for k in ("obs", "mask", "visits", "z", "sym", "prio", "total"):
        P.same_batch(P.run_batch(cpu, ring, prio, index, 130, 511, SEED, BASE, 2, 0, skip=(k,)), exp, skip=(k,))
    bare = dict(ring, obs=None)
    got = P.run_batch(cpu, bare, prio, index, 130, 511, SEED, BASE, 2, 0)
    assert "obs" not in got
    P.same_batch(got, P.batch(bare, prio, False, 130, 511, SEED, BASE, 2, 0))
    a, b = (P.run_batch(cpu, ring, prio, index, 64, 511, SEED, BASE + d, 2, 0) for d in (1, 0))
    assert all(np.array_equal(a[k][:63], b[k][1:]) for k in a if k != "total")   # sample_base shifts it
    assert not np.array_equal(b["index"], P.run_batch(cpu, ring, prio, index, 64, 511, SEED, BASE, 3, 0)["index"])
    assert not np.array_equal(b["index"], R.run_batch(cpu, ring, 64, 511, SEED, BASE, 2, 0)["index"])   # (another stream than the uniform draw's)


def test_a_stale_index_gives_failed_samples(cpu):
    """An append after the build: the index's first word is no longer state[0]."""
    w = R.real_window("time")
    ring, prio = R.new_ring(300), np.zeros(300, np.int32)
    R.run_append(cpu, ring, w, 1)
    P.run_prio_append(cpu, ring, prio, w, None, 4)
    index = P.run_index(cpu, ring, prio)
    live = int(ring["state"][0])
    assert P.run_batch(cpu, ring, prio, index, 65, 511, SEED, BASE, 0, 0)["total"].tolist() == [4 * live, live]
    R.run_append(cpu, ring, w, 2)
    P.run_prio_append(cpu, ring, prio, w, None, 4)
    got = P.run_batch(cpu, ring, prio, index, 65, 511, SEED, BASE, 0, 0)
    P.same_batch(got, P.batch(ring, prio, True, 65, 511, SEED, BASE, 0, 0))
    assert (got["index"] == -1).all() and got["total"].tolist() == [0, min(2 * live, 300)] and not got["prio"].any() and (got["z"] == R.Z_OPEN).all()
    P.same_batch(P.run_batch(cpu, ring, prio, P.run_index(cpu, ring, prio), 65, 511, SEED, BASE, 0, 0),
                 P.batch(ring, prio, False, 65, 511, SEED, BASE, 0, 0))


def test_frequencies_on_a_small_ring(cpu):
    """8 live rows of weights 0 .. 7, 28 x 1 024 samples: the row of weight 0 is never drawn, every other count lies within 5 standard
    deviations (binomial: sqrt(n p (1 - p))) of 1 024 w.  FREQUENCY_SEED makes the restatement alone satisfy this."""
    n = 28 * 1024
    for capacity, total in ((8, 8), (8, 13), (20, 8)):
        ring = ring_at(capacity, total, observations=False)
        prio = np.full(capacity, 1 << 20, np.int32)   # (garbage where the ring is not live)
        slots = [(total - 8 + q) % capacity for q in range(8)]
        prio[slots] = np.arange(8)
        exp = P.batch(ring, prio, False, n, 0, FREQUENCY_SEED, 0, 0, 0)
        count = np.bincount(exp["index"][:, 0], minlength=capacity)
        assert exp["total"].tolist() == [28, 8] and count[slots[0]] == 0 and count.sum() == count[slots].sum() == n
        for w in range(1, 8):
            p = w / 28
            assert abs(int(count[slots[w]]) - 1024 * w) <= 5 * np.sqrt(n * p * (1 - p)), (capacity, total, w, count[slots].tolist())
        got = P.run_batch(cpu, ring, prio, P.run_index(cpu, ring, prio), n, 0, FREQUENCY_SEED, 0, 0, 0)
        P.same_batch(got, exp)


# ---- gbl_cpu_replay_prio_append ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["time", "tile"])
def test_prio_append_host_flavour_equals_restatement(cpu, layout):
    w = R.real_window(layout)
    K = R.count_valid(w)
    cells = w["z"].shape[0]
    per_cell = np.random.default_rng(5).integers(-50, 1000, cells).astype(np.int32)
    for capacity in (K + 7, K - 1, 1, K + K // 2):   # larger than K, one row cut, one slot, and one that the second append wraps
        for prio_traj, value in ((None, 6), (per_cell, 0)):
            ring = R.new_ring(capacity, observations=False)
            got = np.full(capacity, P.FILL, np.int32)
            exp = got.copy()
            for g in range(2 if capacity == K + K // 2 else 1):
                R.run_append(cpu, ring, w, g)
                P.run_prio_append(cpu, ring, got, w, prio_traj, value + g)
                P.prio_append(ring, exp, w, prio_traj, value + g)
                assert np.array_equal(got, exp), (capacity, g, np.argwhere(got != exp)[:5])
            written = min(K, capacity) if capacity != K + K // 2 else capacity
            assert int((got != P.FILL).sum()) == written   # (slots outside the append keep the fill)
            if prio_traj is None and capacity == K + K // 2:
                assert sorted(set(got.tolist())) == [6, 7] and got[(2 * K - 1) % capacity] == 7
    valid = S.valid_cells(w)
    t, b = (x[-1] for x in np.nonzero(valid))   # the newest row is the last valid cell's
    ring, got = R.new_ring(1, observations=False), np.full(1, P.FILL, np.int32)
    R.run_append(cpu, ring, w, 0)
    P.run_prio_append(cpu, ring, got, w, per_cell, 0)
    assert got[0] == per_cell[S.cell(t, b, w["ply_stride"], w["tile_stride"])]


# ---- gbl_cpu_replay_prio_update ----------------------------------------------------------------------------------------------------
def test_prio_update_host_flavour(cpu):
    prio = np.full(10, 100, np.int32)
    index = np.array([[3, 0], [3, 0], [-1, -1], [10, 0], [7, 5], [3, 1], [0, 0], [1 << 30, 0]], np.int32)
    values = np.array([5, 9, 77, 78, -4, 2, 0, 79], np.int32)
    exp = prio.copy()
    P.prio_update(exp, index, values)
    P.run_prio_update(cpu, prio, index, values)
    assert np.array_equal(prio, exp) and prio.tolist() == [0, 100, 100, 9, 100, 100, 100, -4, 100, 100]   # the maximum wins, the old 100 is gone
    P.run_prio_update(cpu, prio, index[:0], values[:0])   # batch 0
    assert np.array_equal(prio, exp)
    rng = np.random.default_rng(1)
    prio, index = rng.integers(-5, 5, 50).astype(np.int32), np.stack([rng.integers(-2, 52, 400), rng.integers(0, 9, 400)], 1).astype(np.int32)
    values = rng.integers(-1000, 1000, 400).astype(np.int32)
    exp = prio.copy()
    P.prio_update(exp, index, values)
    P.run_prio_update(cpu, prio, index, values)
    assert np.array_equal(prio, exp)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_replay_prio_argument_errors_replay_the_recorded_table(golden_dir):
    """tests/golden/replay_prio_arg_errors.json: bad calls of the four entry points with the return code and the gbl_last_error text of
    either flavour (recorded results).  Every call returns before any device work; a case whose "host" is null is an alignment rule."""
    table = json.load(open(os.path.join(golden_dir, "replay_prio_arg_errors.json")))
    assert len(table) > 40 and {c["fn"] for c in table} == {"replay_prio_append", "replay_prio_update", "replay_prio_index", "replay_batch_prio"}
    assert {c["device"][0] for c in table} == {0, nat.ERR_ARG, nat.ERR_ALIGN}
    replay_arg_errors(table)
    L = nat.lib()
    assert [L.gbl_replay_prio_index_bytes(c) for c in (0, -1, 1, 32, 33, 1 << 31, (1 << 31) - 1)] == [0, 0, 40, 40, 48, 0, 8 * (2 + (1 << 20) + 1 + (1 << 26))]


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def collected():
    env = G.BatchedGobblet(130, "cpu", auto_reset=True, seed=5, track_turn=True)
    traj = env.collect(6, policies=("tree", "tree"), search=S.SEARCH)
    env.outcome_targets(traj)
    return env, traj


def numpy_ring(buf):
    ring = {"obs": np.zeros((buf.capacity, 128), np.int8), "visits": np.zeros((buf.capacity, 64), np.int16),
            "meta": np.zeros((buf.capacity, 64), np.int8), "state": np.array([buf.total, 0], np.uint64), "capacity": buf.capacity}
    ring["obs"][:, :117], ring["visits"][:, :54] = buf.observation.numpy(), buf.visits.numpy()
    ring["meta"][:, :54], ring["meta"][:, R.META_Z], ring["meta"][:, R.META_MOVER] = buf.action_mask.numpy(), buf.z.numpy(), buf.mover.numpy()
    ring["meta"][:, R.META_TAG:R.META_TAG + 4] = buf.tag.numpy().astype("<i4").view(np.int8).reshape(-1, 4)
    return ring


KEYS = (("observation", "obs"), ("action_mask", "mask"), ("visits", "visits"), ("z", "z"), ("index", "index"), ("sym", "sym"),
        ("priority", "prio"), ("prio_total", "total"))


def same_as_rule(buf, out, batch, sym_mask, seed, call, recent):
    exp = P.batch(numpy_ring(buf), buf.priority.numpy(), False, batch, sym_mask, seed, 0, call, recent)
    for k, r in KEYS:
        assert np.array_equal(out[k].numpy().astype(exp[r].dtype), exp[r]), k
    return exp


def test_prioritized_buffer_on_the_host_flavour_and_its_stale_index_bookkeeping(collected):
    env, traj = collected
    buf = G.ReplayBuffer(150, "cpu", prioritized=True)
    assert buf.priority.shape == (150,) and buf.priority.dtype == torch.int32 and not buf.priority.any()
    out = buf.batch(40, prioritized=True)   # an empty buffer
    assert (out["index"] == -1).all() and out["prio_total"].tolist() == [0, 0] and out["prio_total"].dtype == torch.int64
    buf.append(env, traj, tag=4, priority=3)
    K = buf.total
    assert 75 < K < 150 and (buf.priority[:K] == 3).all() and not buf.priority[K:].any()
    out = buf.batch(200, symmetries="square", call=2, seed=11, prioritized=True)
    assert same_as_rule(buf, out, 200, 7, 11, 2, 0)["total"].tolist() == [3 * K, K]
    # a per-cell tensor in the window's own layout: the regret-style table look-up; after this append the draw sees the new weights
    cells = (torch.arange(traj["z"].numel(), dtype=torch.int64).reshape(traj["z"].shape) % 5).to(torch.int8) - 1
    table = torch.tensor([0, 1, 4, 8, 6], dtype=torch.int32)
    buf.append(env, traj, tag=5, priority=table[cells.long() + 1])
    ring, prio = R.new_ring(150), np.zeros(150, np.int32)
    w = S.window_of(traj, 130)
    full = np.zeros(w["z"].shape[0], np.int32)
    t, b = np.meshgrid(np.arange(traj["_plies"]), np.arange(130), indexing="ij")
    full[S.cell(t, b, w["ply_stride"], w["tile_stride"])] = table[cells.long() + 1].numpy()
    for tag, (pt, v) in ((4, (None, 3)), (5, (full, 0))):
        R.append(ring, w, tag)
        P.prio_append(ring, prio, w, pt, v)
    assert np.array_equal(buf.priority.numpy(), prio) and buf.total == 2 * K
    out = buf.batch(200, call=3, seed=11, recent=100, prioritized=True, out=None)
    same_as_rule(buf, out, 200, 511, 11, 3, 100)
    # set_priority: the drawn rows get new values; the next draw sees them
    values = torch.arange(200, dtype=torch.int32) % 7
    before = buf.priority.clone()
    buf.set_priority(out["index"], values)
    exp = before.numpy().copy()
    P.prio_update(exp, out["index"].numpy(), values.numpy())
    assert np.array_equal(buf.priority.numpy(), exp) and not np.array_equal(exp, before.numpy())
    assert buf.batch(200, call=4, seed=11, prioritized=True, out=out) is out
    same_as_rule(buf, out, 200, 511, 11, 4, 0)
    # set_all_priority: one live row left with weight -> every sample is that row
    only = torch.zeros(150, dtype=torch.int32)
    only[77] = 2
    buf.set_all_priority(only)
    out = buf.batch(64, call=5, prioritized=True)
    assert (out["index"][:, 0] == 77).all() and (out["priority"] == 2).all() and out["prio_total"].tolist() == [2, 150]
    same_as_rule(buf, out, 64, 511, 0, 5, 0)
    buf.set_all_priority(torch.zeros(150, dtype=torch.int32))
    assert (buf.batch(64, call=5, prioritized=True)["index"] == -1).all()
    with pytest.raises(ValueError, match="priority"):
        buf.append(env, traj, priority=torch.zeros(3, dtype=torch.int32))
    plain = G.ReplayBuffer(150, "cpu")
    for call in (lambda: plain.priority, lambda: plain.batch(8, prioritized=True), lambda: plain.append(env, traj, priority=2),
                 lambda: plain.set_all_priority(only), lambda: plain.set_priority(out["index"], out["priority"])):
        with pytest.raises(ValueError, match="prioritized=True"):
            call()


def test_importance_weights_against_a_hand_computation():
    batch = {"priority": torch.tensor([1, 2, 4, 0], dtype=torch.int32), "prio_total": torch.tensor([40, 10], dtype=torch.int64)}
    # p = w / 40, span = 10: 1 / (10 p) = 4, 2, 1 and the failed sample 0; normalised by the maximum 4
    assert torch.allclose(G.ReplayBuffer.importance_weights(batch, 1.0), torch.tensor([1.0, 0.5, 0.25, 0.0]), rtol=0, atol=1e-7)
    assert torch.allclose(G.ReplayBuffer.importance_weights(batch, 0.5), torch.tensor([1.0, 0.5 ** 0.5, 0.5, 0.0]), rtol=0, atol=1e-7)
    assert G.ReplayBuffer.importance_weights(batch, 0.0).tolist() == [1.0, 1.0, 1.0, 0.0]
    batch["priority"][:] = 0
    assert G.ReplayBuffer.importance_weights(batch, 1.0).tolist() == [0.0] * 4 and G.ReplayBuffer.importance_weights(batch).dtype == torch.float32


def test_prioritized_fit_equals_the_hand_written_loop_and_state_dict_round_trips(collected):
    env, traj = collected
    buf = G.ReplayBuffer(200, "cpu", prioritized=True)
    buf.append(env, traj, tag=1, priority=1)
    buf.append(env, traj, tag=2, priority=5)
    a, b = G.GobbletTrainer(hidden=64, device="cpu", seed=1), G.GobbletTrainer(hidden=64, device="cpu", seed=1)
    stats = buf.fit(a, 3, batch=256, first_call=7, recent=150, prioritized=True)
    by_hand = torch.stack([b.step(buf.batch(256, call=7 + i, recent=150, prioritized=True)) for i in range(3)])
    assert stats.shape == (3, 4) and torch.equal(stats, by_hand) and float(stats[:, 2].min()) == 256
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    c = G.GobbletTrainer(hidden=64, device="cpu", seed=1)
    assert not torch.equal(buf.fit(c, 3, batch=256, first_call=7, recent=150), stats)   # (the uniform fit is another one)
    state = buf.state_dict()
    assert set(state) == {"capacity", "observations", "state", "visits", "meta", "obs", "priority"}
    other = G.ReplayBuffer(200, "cpu", prioritized=True)
    other.load_state_dict(state)
    x, y = buf.batch(200, call=3, seed=9, prioritized=True), other.batch(200, call=3, seed=9, prioritized=True)
    assert all(torch.equal(x[k], y[k]) for k in x) and (x["index"][:, 0] >= 0).all() and torch.equal(other.priority, buf.priority)
    buf.set_all_priority(torch.ones(200, dtype=torch.int32))   # (the state is a copy)
    assert not torch.equal(other.priority, buf.priority)
    plain = G.ReplayBuffer(200, "cpu")
    plain.load_state_dict(state)   # the ring of a prioritised buffer loads into a plain one; the reverse has no priorities to offer
    with pytest.raises(ValueError, match="priorities"):
        other.load_state_dict(plain.state_dict())


def test_an_unprioritized_buffer_is_what_it_was(cpu, collected):
    env, traj = collected
    buf = G.ReplayBuffer(150, "cpu")
    buf.append(env, traj, tag=4)
    buf.append(env, traj, tag=5)
    assert not buf.prioritized and not hasattr(buf, "_prio") and not hasattr(buf, "_index")
    assert set(buf.state_dict()) == {"capacity", "observations", "state", "visits", "meta", "obs"}
    out = buf.batch(300, symmetries="all", call=4, seed=11, recent=50)
    assert set(out) == {"observation", "action_mask", "visits", "z", "index", "sym"}
    exp = R.run_batch(cpu, numpy_ring(buf), 300, 511, 11, 0, 4, 50)   # the existing gbl_replay_batch call
    for k, r in KEYS[:6]:
        assert np.array_equal(out[k].numpy(), exp[r]), k
    both = G.ReplayBuffer(150, "cpu", prioritized=True)
    both.append(env, traj, tag=4)
    both.append(env, traj, tag=5)
    same = both.batch(300, symmetries="all", call=4, seed=11, recent=50)   # the uniform draw of a prioritised buffer is the same draw
    assert set(same) == set(out) and all(torch.equal(same[k], out[k]) for k in out)


def test_the_prioritized_example_runs_on_the_host_flavour():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_prioritized_replay", os.path.join(root, "examples", "example_prioritized_replay.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    log = ex.prioritized_replay("cpu", inventory=(2, 2, 0), windows=2, boards=128, plies=12, steps=3, batch=128, iterations=8, capacity=2048,
                                held_out=256)
    assert set(log) == {"uniform", "prioritized", "rows", "weight_by_class"} and log["rows"] > 0
    assert sum(log["weight_by_class"].values()) > log["rows"] and log["uniform"]["rows"] == log["prioritized"]["rows"] > 0
    assert all(0.0 <= log[k][s] <= 1.0 for k in ("uniform", "prioritized") for s in ("value_sign", "top_prior_in_R"))
