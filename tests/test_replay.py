"""The replay buffer, host flavour (no GPU): gbl_cpu_replay_append and gbl_cpu_replay_batch against the numpy restatement of the
header's paragraph (tests/replay_restatement.py) -- the whole ring with its padding and its state after every append, every output of
every draw --, the drawn rows against gbl_cpu_symmetry_apply on the stored rows, the exactness of the draw on a small ring,
ReplayBuffer on the host flavour (fit against the hand-written loop, state_dict) and the recorded argument errors."""
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import replay_restatement as R
from tests import symmetry_restatement as S
from tests.search_harness import replay_arg_errors

SEED, BASE = 0x1234567890ABCDEF, (1 << 40) + 5
WINDOWS = {"real-time": lambda: R.real_window("time"), "real-tile": lambda: R.real_window("tile"), "all": lambda: R.synthetic("all"),
           "none": lambda: R.synthetic("none"), "checkerboard": lambda: R.synthetic("checkerboard")}


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


def both(cpu, ring, w, tag):
    """One append by the library and by the restatement on copies of `ring`, compared; returns the ring after it and K."""
    got, exp = R.copy_ring(ring), R.copy_ring(ring)
    R.run_append(cpu, got, w, tag)
    K = R.append(exp, w, tag)
    R.same_ring(got, exp)
    return got, K


# ---- append ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WINDOWS))
def test_append_host_flavour_equals_restatement(cpu, name):
    w = WINDOWS[name]()
    K = R.count_valid(w)
    assert (name == "none") == (K == 0)
    if name.startswith("real"):
        assert 50 < K < 130 * 5 and (w["tile_stride"] == 64) == (name == "real-time")
    if name == "all":
        assert K == 130 * 4
    for i, capacity in enumerate(sorted({K + 7, max(K, 1), max(K - 1, 1), 1})):   # larger than K, exactly K, one row cut, one slot
        for observations in (True, False):
            ring, k = both(cpu, R.new_ring(capacity, observations, junk=i), w, 3 + i)
            assert k == K and ring["state"].tolist() == [K, K]
            if K >= capacity:   # the ring is full of this window's last rows: nothing of the junk is left, and the newest row is the last cell
                t, b = (x[-1] for x in np.nonzero(S.valid_cells(w)))
                at = S.cell(t, b, w["ply_stride"], w["tile_stride"])
                assert np.array_equal(ring["visits"][(K - 1) % capacity, :54], w["visits"][at]) and (ring["meta"][:, R.META_TAG] == 3 + i).all()
    if K == 0:
        return
    # two appends whose second wraps the end; three whose total passes twice the capacity; a T0 beyond 2^32
    for capacity, times in ((K + K // 2, 2), (K + K // 3, 3)):
        ring = R.new_ring(capacity, junk=9)
        for g in range(times):
            ring, _ = both(cpu, ring, w, -g)
        assert ring["state"].tolist() == [times * K, K] and (times == 2 or times * K > 2 * capacity)
        assert set(ring["meta"][:, R.META_TAG:R.META_TAG + 4].copy().view("<i4")[:, 0].tolist()) == {-(times - 1), -(times - 2)}
    ring = R.new_ring(K + 5, junk=10)
    ring["state"][0] = (1 << 40) + 3
    ring, _ = both(cpu, ring, w, 1 << 30)
    assert int(ring["state"][0]) == (1 << 40) + 3 + K


def test_append_leaves_everything_else_alone(cpu):
    """A checkerboard window into a ring twice its size: the slots beyond the K written ones keep their junk, byte for byte."""
    w = R.synthetic("checkerboard")
    K = R.count_valid(w)
    before = R.new_ring(2 * K, junk=4)
    after, _ = both(cpu, before, w, 7)
    for k in ("obs", "visits", "meta"):
        assert np.array_equal(after[k][K:], before[k][K:]) and not np.array_equal(after[k][:K], before[k][:K])
    assert not after["obs"][:K, 117:].any() and not after["visits"][:K, 54:].any() and not after["meta"][:K, 60:].any()


# ---- batch -------------------------------------------------------------------------------------------------------------------------
def filled_ring(cpu, capacity, observations=True, times=1):
    ring = R.new_ring(capacity, observations, junk=1)
    for g in range(times):
        R.run_append(cpu, ring, R.real_window("time" if g % 2 == 0 else "tile"), 100 + g)
    return ring


@pytest.mark.parametrize("capacity,times", [(1000, 1), (200, 2)])
def test_batch_host_flavour_equals_restatement(cpu, capacity, times):
    ring = filled_ring(cpu, capacity, times=times)
    live = min(int(ring["state"][0]), capacity)
    assert (live == capacity) == (times == 2)
    for sym_mask in (0, 7, 511):
        for recent in (0, 1, 5, live + 10):
            exp = R.batch(ring, 300, sym_mask, SEED, BASE, 3, recent)
            for n in (1, 63, 65, 300):   # a batch is the beginning of every longer one
                R.same_batch(R.run_batch(cpu, ring, n, sym_mask, SEED, BASE, 3, recent), exp, n)
            span = live if recent in (0, live + 10) else recent
            age = (int(ring["state"][0]) - 1 - exp["index"][:, 0]) % capacity
            assert 0 <= age.min() and age.max() < span and (span > 5 or set(age.tolist()) == set(range(span)))
            assert exp["sym"].max() <= sym_mask and (sym_mask == 0 or len(set(exp["sym"].tolist())) > min(sym_mask, 200) * 0.7)
            assert set(exp["index"][:, 1].tolist()) <= {100, 101}
    a, b = R.run_batch(cpu, ring, 64, 511, SEED, BASE + 1, 0, 0), R.run_batch(cpu, ring, 64, 511, SEED, BASE, 0, 0)
    assert all(np.array_equal(a[k][:63], b[k][1:]) for k in a)   # sample_base shifts it
    assert not np.array_equal(b["index"], R.run_batch(cpu, ring, 64, 511, SEED, BASE, 1, 0)["index"])
    assert not np.array_equal(b["index"], R.run_batch(cpu, ring, 64, 511, SEED + 1, BASE, 0, 0)["index"])


@pytest.mark.parametrize("capacity", [33, 1000])
def test_batch_of_a_ring_that_has_taken_more_than_2_to_the_32_rows(cpu, capacity):
    """ring_state[0] is a uint64 count of rows ever appended: the newest slot is (total - 1) mod capacity in 64 bits.  None of the three
    totals gives the same slot when it is cut to 32 bits first (asserted), and one `recent` reaches back across slot 0."""
    crossed = False
    for total in ((1 << 32) + 5, 3 * (1 << 32) + capacity // 2, (1 << 40) + 3):
        ring = R.new_ring(capacity, junk=capacity)
        ring["meta"][:, R.META_MOVER] &= 1
        ring["state"][0] = total
        newest = (total - 1) % capacity
        assert newest != ((total - 1) & 0xFFFFFFFF) % capacity
        for recent in (0, 7, capacity - 1):
            exp = R.batch(ring, 65, 511, SEED, BASE, 3, recent)
            R.same_batch(R.run_batch(cpu, ring, 65, 511, SEED, BASE, 3, recent), exp)
            span = recent if recent else capacity
            age = (newest - exp["index"][:, 0]) % capacity
            assert age.max() < span and (span > 7 or set(age.tolist()) == set(range(span)))
            crossed |= recent > newest + 1 and bool((exp["index"][:, 0] > newest).any())
    assert crossed


def test_batch_of_an_empty_buffer_and_of_one_without_observations(cpu):
    empty = R.new_ring(50, junk=2)
    got = R.run_batch(cpu, empty, 65, 511, 1, 0, 0, 0)
    R.same_batch(got, R.batch(empty, 65, 511, 1, 0, 0, 0))
    assert not got["obs"].any() and not got["mask"].any() and not got["visits"].any() and not got["sym"].any()
    assert (got["index"] == -1).all() and (got["z"] == R.Z_OPEN).all()
    bare, full = filled_ring(cpu, 1000, observations=False), filled_ring(cpu, 1000)
    got = R.run_batch(cpu, bare, 200, 511, 2, 0, 5, 0)
    assert "obs" not in got
    R.same_batch(got, R.batch(bare, 200, 511, 2, 0, 5, 0))
    exp = R.run_batch(cpu, full, 200, 511, 2, 0, 5, 0)
    assert all(np.array_equal(got[k], exp[k]) for k in got)


def test_drawn_rows_are_the_symmetry_entry_points_images_of_the_stored_rows(cpu):
    ring = filled_ring(cpu, 200, times=2)
    got = R.run_batch(cpu, ring, 500, 511, SEED, 0, 9, 0)
    slot = got["index"][:, 0]
    meta = ring["meta"][slot]
    img = S.run_apply(cpu, got["sym"], meta[:, R.META_MOVER], obs=ring["obs"][slot][:, :117], mask=meta[:, :54], visits=ring["visits"][slot][:, :54])
    for k in ("obs", "mask", "visits"):
        assert np.array_equal(img[k], got[k]), k
    assert np.array_equal(got["z"], meta[:, R.META_Z]) and (got["z"] != R.Z_OPEN).all() and len(set(got["sym"].tolist())) > 200
    assert set(meta[:, R.META_MOVER].tolist()) == {0, 1}


def test_the_draw_is_exact_on_a_small_ring(cpu):
    """8 live rows: 1 024 samples hit each of the 8 slots and no other; with recent = 3 the newest three only (fixed seed)."""
    w = R.real_window("time")
    for capacity, total_before in ((8, 0), (8, 5), (20, 0)):   # a full ring, one whose newest row is mid-ring, one with 8 of 20 slots live
        ring = R.new_ring(capacity, junk=3)
        ring["state"][0] = total_before
        if capacity == 20:   # eight rows only: a window with eight valid cells
            valid = np.zeros((3, 70), bool)
            valid[1, 3:7] = valid[2, 60:64] = True
            w8 = S.synthetic_window(70, 3, valid)
            R.run_append(cpu, ring, w8, 1)
            assert ring["state"].tolist() == [8, 8]
        else:
            R.run_append(cpu, ring, w, 1)
        total = int(ring["state"][0])
        got = R.run_batch(cpu, ring, 1024, 511, 42, 0, 0, 0)
        live = sorted((total - 1 - a) % capacity for a in range(8))
        assert sorted(set(got["index"][:, 0].tolist())) == live
        assert np.bincount(got["index"][:, 0], minlength=capacity)[live].min() > 80   # (128 expected per slot)
        got = R.run_batch(cpu, ring, 1024, 511, 42, 0, 0, 3)
        assert sorted(set(got["index"][:, 0].tolist())) == sorted((total - 1 - a) % capacity for a in range(3))


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def collected(boards=130, plies=6, seed=5):
    env = G.BatchedGobblet(boards, "cpu", auto_reset=True, seed=seed, track_turn=True)
    traj = env.collect(plies, policies=("tree", "tree"), search=S.SEARCH)
    return env, traj


def test_replay_buffer_on_the_host_flavour(cpu):
    env, traj = collected()
    buf = G.ReplayBuffer(150, "cpu")
    assert buf.size == 0 == buf.total and buf.observation.shape == (150, 117) and buf.tag.dtype == torch.int32
    with pytest.raises(ValueError, match="outcome_targets"):
        buf.append(env, traj)
    env.outcome_targets(traj)
    assert buf.append(env, traj, tag=4) is None
    w = S.window_of(traj, 130)
    ring = R.new_ring(150)
    K = R.append(ring, w, 4)
    assert buf.size == K == buf.total and 75 < K < 150
    for name, exp in (("observation", ring["obs"][:, :117]), ("action_mask", ring["meta"][:, :54]), ("visits", ring["visits"][:, :54]),
                      ("z", ring["meta"][:, R.META_Z]), ("mover", ring["meta"][:, R.META_MOVER])):
        assert np.array_equal(getattr(buf, name).numpy(), exp), name
    assert (buf.tag[:K] == 4).all() and not buf.tag[K:].any()
    buf.append(env, traj, tag=5)
    R.append(ring, w, 5)
    assert buf.total == 2 * K and buf.size == 150
    for symmetries, sym_mask in (("all", 511), ("square", 7), (None, 0)):
        for recent in (None, 50):
            out = buf.batch(300, symmetries=symmetries, call=4, seed=11, recent=recent)
            exp = R.batch(ring, 300, sym_mask, 11, 0, 4, recent or 0)
            for k, r in (("observation", "obs"), ("action_mask", "mask"), ("visits", "visits"), ("z", "z"), ("index", "index"), ("sym", "sym")):
                assert np.array_equal(out[k].numpy(), exp[r]), (symmetries, recent, k)
    assert buf.batch(300, symmetries=None, call=4, out=out) is out
    with pytest.raises(ValueError, match="out"):
        buf.batch(299, out=out)
    with pytest.raises(ValueError):
        buf.batch(8, symmetries="diagonal")
    with pytest.raises(ValueError):
        G.ReplayBuffer(0, "cpu")
    bare = G.ReplayBuffer(150, "cpu", observations=False)
    bare.append(env, traj)
    assert bare.observation is None and set(bare.batch(8)) == {"action_mask", "visits", "z", "index", "sym"}
    with pytest.raises(ValueError, match="observation"):
        G.GobbletTrainer(hidden=64, device="cpu").step(bare.batch(8))


def test_fit_equals_the_hand_written_loop_and_state_dict_round_trips():
    env, traj = collected()
    env.outcome_targets(traj)
    buf = G.ReplayBuffer(200, "cpu")
    buf.append(env, traj, tag=1)
    buf.append(env, traj, tag=2)
    a, b = G.GobbletTrainer(hidden=64, device="cpu", seed=1), G.GobbletTrainer(hidden=64, device="cpu", seed=1)
    stats = buf.fit(a, 3, batch=256, symmetries="all", first_call=7, recent=100)
    by_hand = torch.stack([b.step(buf.batch(256, symmetries="all", call=7 + i, recent=100)) for i in range(3)])
    assert stats.shape == (3, 4) and torch.equal(stats, by_hand) and float(stats[:, 2].min()) == 256
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert buf.fit(a, 0).shape == (0, 4)
    state = buf.state_dict()
    other = G.ReplayBuffer(200, "cpu")
    other.load_state_dict(state)
    assert other.total == buf.total > 200 and other.size == 200
    x, y = buf.batch(200, call=3, seed=9), other.batch(200, call=3, seed=9)
    assert all(torch.equal(x[k], y[k]) for k in x) and (x["index"][:, 0] >= 0).all()
    buf.append(env, traj, tag=3)   # (the state is a copy: the first buffer moves on alone)
    assert other.total != buf.total
    with pytest.raises(ValueError):
        G.ReplayBuffer(400, "cpu").load_state_dict(state)


def test_the_replay_example_runs_on_the_host_flavour():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_replay_loop", os.path.join(root, "examples", "example_replay_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    log = ex.replay_loop("cpu", generations=2, boards=128, plies=16, steps=2, batch=128, hidden=64, iterations=8, capacity=400, arena_boards=64)
    assert len(log) == 2 and log[1]["total"] > log[0]["total"] > 0 and log[1]["size"] == min(log[1]["total"], 400)
    assert all(np.isfinite(g["policy_loss"]) and 0.0 <= g["arena_score"] <= 1.0 for g in log)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_replay_argument_errors_replay_the_recorded_table(golden_dir):
    """tests/golden/replay_arg_errors.json: bad calls of gbl_replay_append and gbl_replay_batch with the return code and the
    gbl_last_error text of either flavour (written from the header).  Every call returns before any device work (the pointers are numbers,
    never read); a case whose "host" is null is an alignment rule, which only the device flavour has."""
    table = json.load(open(os.path.join(golden_dir, "replay_arg_errors.json")))
    assert len(table) > 40 and {c["fn"] for c in table} == {"replay_append", "replay_batch"}
    replay_arg_errors(table)
    L = nat.lib()
    assert L.gbl_replay_workspace_bytes(130, 6) == 32 + 16 * 5 * 3 == R.workspace_bytes(130, 6)
    assert [L.gbl_replay_workspace_bytes(*a) for a in ((0, 6), (130, 1), (130, 32768), ((1 << 31) + 1, 6))] == [0, 0, 0, 0]
