"""The replay stack past 32 bits on the MI355X (-m gpu): ring_state[0] beyond 2^33, rows whose byte offsets pass 2^31 and 2^32, and a
priority ring of more blocks than k_replay_prio_leaves has workgroups.

The huge rings (10 and 12 GiB) are zero-filled on the device and never copied to the host.  Their reference is a SMALL ring of exactly K
slots, K the window's valid rows, which the host flavour fills from state[0] = 0 (tests/test_replay.py and tests/test_replay_prio.py hold
the host flavour to the restatement of the header).  By the append rule, slot (T0 + r) mod capacity of the big ring is slot r of the small
one byte for byte, and a draw over the newest K rows is the small ring's draw over everything with the slots translated.  The index of
the largest priority ring is compared with the host flavour's word for word (tests/test_replay_prio.py holds that one to its layout)."""
import numpy as np
import pytest
import torch

from tests import replay_prio_restatement as P
from tests import replay_restatement as R
from tests import symmetry_restatement as S
from tests.search_harness import G  # noqa: F401  (the fixture)
from tests.test_gpu_replay import DEV, device_append, on_device
from tests.test_gpu_replay import device_batch as device_batch_uniform
from tests.test_gpu_replay_prio import BASE, SEED, device_batch, device_index, device_prio_append, tile_major

pytestmark = pytest.mark.gpu

LINE = 128
PITCH = {"obs": R.OBS_PITCH, "visits": 2 * R.VISITS_PITCH, "meta": R.META_PITCH, "prio": 4}   # bytes per row
VIEW = {"obs": np.int8, "visits": np.int16, "meta": np.int8, "prio": np.int32}


class Lines:
    """`nbytes` zero bytes on the device that start on a 128-byte line (as gobblet_rl_amd.replay._lines), never copied whole."""

    def __init__(self, nbytes):
        raw = torch.zeros(nbytes + LINE, dtype=torch.uint8, device=DEV)
        lead = -raw.data_ptr() % LINE
        self.bytes = raw[lead:lead + nbytes]
        self.ptr = self.bytes.data_ptr()
        assert self.ptr % LINE == 0


class BigRing:
    """DeviceRing's surface (capacity, a, ptr, ws) over zero-filled device arrays; `prio` is the ring's priorities (Guarded's surface).
    rows=False: the state and the priorities alone."""

    def __init__(self, capacity, observations=True, rows=True):
        self.capacity = capacity
        self.a = {k: Lines(capacity * PITCH[k]) for k in ("obs", "visits", "meta") if rows and (k != "obs" or observations)}
        self.a["state"] = Lines(16)
        self.prio = Lines(capacity * 4)

    def ptr(self, k):
        return self.a[k].ptr if k in self.a else None

    def lines(self, k):
        return self.prio if k == "prio" else self.a[k]

    def runs(self, k, start, count):
        """The rows (start + i) mod capacity, i < count, of array k as one or two slices (no index arithmetic but the slice's own)."""
        rows = self.lines(k).bytes.view(self.capacity, PITCH[k])
        start %= self.capacity
        stop = min(start + count, self.capacity)
        return [rows[start:stop]] + ([rows[:start + count - stop]] if stop < start + count else [])

    def rows(self, k, start, count):
        """Those rows on the host, in the small ring's dtype and shape."""
        got = torch.cat(self.runs(k, start, count)).cpu().numpy()
        return got.view(np.int32).reshape(-1) if k == "prio" else got.view(VIEW[k]).reshape(count, -1)

    def clear(self, k, start, count):
        for run in self.runs(k, start, count):
            run.zero_()

    def words_set(self, k):
        """How many of the array's 8-byte words (of the priorities: how many of them) are not zero.  Counted 256 MiB at a time: the
        reduction's temporary is as large as what it is given."""
        words = self.lines(k).bytes.view(torch.int32 if k == "prio" else torch.int64)
        return int(sum(torch.count_nonzero(part) for part in words.split(1 << 25)))

    def set_state(self, total):
        self.a["state"].bytes.view(torch.int64).copy_(torch.tensor([total, 0], dtype=torch.int64))

    def state(self):
        return self.a["state"].bytes.view(torch.int64).cpu().tolist()


def words_set(a):
    """The same count over a numpy array whose rows are whole 8-byte words."""
    return int(np.count_nonzero(np.ascontiguousarray(a).reshape(-1).view(np.int64)))


@pytest.fixture(scope="module")
def windows(G):
    """257 boards x 5 plies, about 60 % of the cells valid, in both layouts, with near-maximum per-cell priorities and some zeros; for
    either kind of ring the small ring of exactly K slots that the host flavour fills from state[0] = 0, its priorities and its index."""
    cpu = G._native.cpu_raw()
    valid = np.random.default_rng(257).random((5, 257)) < 0.6
    valid[0] = False
    K = int(valid.sum())
    assert 550 < K < 700
    out = {"K": K}
    for layout in ("time", "tile"):
        w = S.synthetic_window(257, 5, valid, seed=5)
        w = tile_major(w) if layout == "tile" else w
        rng = np.random.default_rng(7)
        per_cell = ((1 << 31) - 1 - rng.integers(0, 1000, w["z"].shape[0])).astype(np.int32)
        per_cell[rng.random(len(per_cell)) < 0.25] = 0
        out[layout] = {"w": w, "per_cell": per_cell}
        for observations in (True, False):
            small, sprio = R.new_ring(K, observations), np.zeros(K, np.int32)
            R.run_append(cpu, small, w, TAG)
            P.run_prio_append(cpu, small, sprio, w, per_cell, 0)
            assert small["state"].tolist() == [K, K] and (sprio > 0).sum() > K // 2 and (sprio == 0).sum() > K // 8
            out[layout][observations] = (small, sprio, P.run_index(cpu, small, sprio))
    return out


TAG = (1 << 30) + 77
# capacity, observations, and per append (m, first slot as a function of K): T0 = m capacity + first >= 2^33.  Ring A: the rows straddle
# slot 2^24 (obs and visits offsets cross 2^31), slot 2^25 (they cross 2^32, the meta offset 2^31; the rows end 7 slots before the
# ring's end) and the ring's end (they wrap to slot 0).  Ring B: slot 2^26 (the meta offset crosses 2^32) and the ring's end.
CAP_A, CAP_B = (1 << 25) + 97, (1 << 26) + 97
RINGS = {
    "A": (CAP_A, True, [(257, lambda K: (1 << 24) - K // 2), ((1 << 40) // CAP_A + 1, lambda K: (1 << 25) + 90 - K),
                        ((1 << 52) // CAP_A + 3, lambda K: CAP_A - K // 2)]),
    "B": (CAP_B, False, [(129, lambda K: (1 << 26) + 90 - K), ((1 << 47) // CAP_B + 5, lambda K: CAP_B - K // 3)]),
}


@pytest.mark.parametrize("layout", ["time", "tile"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_appends_and_draws_on_a_ring_past_32_bits(G, windows, name, layout):
    """Per append of RINGS[name]: gbl_replay_append, gbl_replay_prio_append and the index on one stream at state[0] = T0; then the written
    rows, their surroundings, the count of everything set, the state, and draws of both kinds against the small ring.  An allocation that
    fails fails the test."""
    torch.cuda.empty_cache()   # (the two rings are never resident together)
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    capacity, observations, appends = RINGS[name]
    K, w, per_cell = windows["K"], windows[layout]["w"], windows[layout]["per_cell"]
    small, sprio, sindex = windows[layout][observations]
    arrays = [k for k in ("obs", "visits", "meta") if small[k] is not None]
    wd, per_cell_dev = on_device(w), torch.from_numpy(per_cell).to(DEV)
    ring = BigRing(capacity, observations)
    for m, first_of in appends:
        first = first_of(K)
        T0 = m * capacity + first
        assert T0 >= 1 << 33 and T0 % capacity == first and 0 < first < capacity
        ring.set_state(T0)
        device_append(lib, ring, w, wd, TAG)
        device_prio_append(lib, ring, ring.prio, w, wd, per_cell_dev, 0)
        index = device_index(lib, ring, ring.prio)
        torch.cuda.synchronize()
        ring.ws.read()   # (its guards)
        assert ring.state() == [T0 + K, K]
        # slot (T0 + r) mod capacity holds the small ring's slot r, the 64 slots on either side nothing, no other word of the array is set
        for k in arrays + ["prio"]:
            got, exp = ring.rows(k, first, K), sprio if k == "prio" else small[k]
            assert got.dtype == exp.dtype and np.array_equal(got, exp), (k, first, np.argwhere(got != exp)[:5])
            assert not ring.rows(k, first - 64, 64).any() and not ring.rows(k, first + K, 64).any(), (k, first)
            assert ring.words_set(k) == (np.count_nonzero(sprio) if k == "prio" else words_set(small[k])), (k, first)
        # the uniform draw over the newest K rows, the weighted one over everything, over the K rows and over 50 weightless rows more
        for batch in (130, 4161):
            exp = R.run_batch(cpu, small, batch, 511, SEED, BASE, 3, 0)
            exp["index"][:, 0] = (T0 + exp["index"][:, 0].astype(np.int64)) % capacity
            R.same_batch(device_batch_uniform(lib, ring, batch, 511, SEED, BASE, 3, K), exp)
            exp = P.run_batch(cpu, small, sprio, sindex, batch, 511, SEED, BASE, 3, 0)
            exp["index"][:, 0] = (T0 + exp["index"][:, 0].astype(np.int64)) % capacity
            assert int(exp["total"][0]) == int(P.weights(sprio).sum()) > 1 << 39 and (exp["prio"] > 0).all()
            for recent in (0, K, K + 50):
                exp["total"][1] = recent if recent else capacity
                P.same_batch(device_batch(lib, ring, ring.prio, index, batch, 511, 3, recent), exp)
        assert index.read()[0] == T0 + K
        for k in arrays + ["prio"]:   # the next append starts from an empty ring again
            ring.clear(k, first, K)
    assert all(ring.words_set(k) == 0 for k in arrays + ["prio"])
    del ring
    torch.cuda.empty_cache()


def test_an_index_of_more_blocks_than_the_leaves_kernel_has_workgroups(G):
    """2^27 + 3 * 2048 + 33 slots: 65 540 blocks, so four workgroups of k_replay_prio_leaves take a second trip round their loop, the last
    leaf is ragged (one slot) and every thread of k_replay_prio_scan walks 65 blocks; priorities near 2^31 - 1, W about 2^57.5.  Only the
    priorities, the state and the index exist.  Wrapped; then state[0] = capacity - 1 (the ragged leaf is not live) and capacity - 3
    (the cut falls inside a 16-byte vector of a second-trip block: its first two entries live, its last two not), with the LARGEST
    weight in every slot that is not live -- an index that counted one of them differs from the host flavour's, which
    tests/test_replay_prio.py holds to the layout at these three states.  Each index built twice into junk.  Then
    gbl_replay_prio_update on the same ring, with slots in the last block."""
    torch.cuda.empty_cache()
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    capacity = (1 << 27) + 3 * 2048 + 33
    assert lib.gbl_replay_prio_index_bytes(capacity) == 8 * (2 + 65540 + 1 + 4194498)
    prio = P.wide_priorities(capacity, 3 * capacity + 1000)
    ring = BigRing(capacity, rows=False)
    dprio = ring.prio
    dprio.bytes.view(torch.int32).copy_(torch.from_numpy(prio))
    assert (capacity - 1) % 32 == 0 and (capacity - 5) % 4 == 0 and (capacity - 5) // 2048 >= 1 << 16
    for total in (3 * capacity + 1000, capacity - 1, capacity - 3):
        if total < capacity:   # behind the newest row garbage that would count if the slot were taken for live
            prio[total:] = (1 << 31) - 1
            dprio.bytes.view(torch.int32)[total:] = (1 << 31) - 1
            assert (prio[capacity - 5:] > 0).all()   # live and dead entries of the last vectors alike
        ring.set_state(total)
        host = {"capacity": capacity, "state": np.array([total, 0], np.uint64)}
        hindex = P.run_index(cpu, host, prio)
        live = min(total, capacity)
        assert int(hindex[1]) == int(np.maximum(prio[:live], 0).sum(dtype=np.int64)) > 1 << 57
        built = [device_index(lib, ring, dprio).read() for _ in range(2)]   # (read: the guards of the exactly-sized block)
        for words in built:
            assert words.dtype == hindex.dtype and np.array_equal(words, hindex), (total, np.argwhere(words != hindex)[:5])
    # gbl_replay_prio_update: slots of the last block and of the first, repeated ones, the last slot, one past it and -1
    rng = np.random.default_rng(4)
    batch = 4096
    slots = np.concatenate([rng.integers(capacity - 2048, capacity, 1500), rng.integers(0, capacity, 1500), rng.integers(0, 64, 1000),
                            [capacity - 1, capacity - 1, capacity, -1]])
    slots = np.concatenate([slots, np.full(batch - len(slots), capacity - 3)])
    index = np.stack([slots, rng.integers(0, 9, batch)], 1).astype(np.int32)
    values = rng.integers(-1000, 1 << 31, batch).astype(np.int32)
    dindex, dvalues = torch.from_numpy(index).to(DEV), torch.from_numpy(values).to(DEV)
    rc = lib.gbl_replay_prio_update(dindex.data_ptr(), dvalues.data_ptr(), batch, dprio.ptr, capacity, None)
    assert rc == 0, lib.gbl_last_error()
    torch.cuda.synchronize()
    P.run_prio_update(cpu, prio, index, values)
    assert torch.equal(dprio.bytes.view(torch.int32).cpu(), torch.from_numpy(prio))
    assert len(set(slots.tolist())) < batch - 100 and (slots >= capacity - 2048).sum() > 1500
    del ring, dprio
    torch.cuda.empty_cache()
