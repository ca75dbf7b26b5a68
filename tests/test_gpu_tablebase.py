"""The tablebase kernels on the MI355X (-m gpu): k_tb_prepare, k_tb_sweep, k_tb_index, k_tb_position and k_tb_probe against the host
flavour byte for byte (which tests/test_tablebase.py holds to the restatement of the header), every output read back through guard
bytes.  Universes: (1, 1, 1), (2, 1, 0), (1, 1, 2) with 11.8 M positions and 43 sweeps -- more positions than one pass of the sweep's
grid -- and (2, 2, 0) for the ragged slices; the full inventory in slices of 4 096 positions at 0, across 2^31 and at the end (an
index needs all 32 bits there; no universe reaches 2^32)."""
import numpy as np
import pytest
import torch

from gobblet_rl_amd import _native as nat
from tests import tablebase_harness as H
from tests.search_harness import G  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, JUNK = 256, 0x5A


class Guarded:
    """A device array of `nbytes` (or holding the numpy array `a`) with GUARD junk bytes on both sides; the payload is 256-byte aligned."""

    def __init__(self, a=None, nbytes=None, lead=0):
        body = np.full(nbytes, JUNK, np.uint8) if a is None else np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        self.nbytes, self.lead = len(body), GUARD + lead
        self.raw = torch.from_numpy(np.concatenate([np.full(self.lead, JUNK, np.uint8), body, np.full(GUARD, JUNK, np.uint8)])).to(DEV)

    @property
    def ptr(self):
        return self.raw.data_ptr() + self.lead

    def body(self):
        """The payload as a device tensor (int8)."""
        return self.raw[self.lead:self.lead + self.nbytes].view(torch.int8)

    def read(self, dtype=np.int8, shape=None):
        raw = self.raw.cpu().numpy()
        assert (raw[:self.lead] == JUNK).all() and (raw[self.lead + self.nbytes:] == JUNK).all(), "a guard byte was written"
        out = raw[self.lead:self.lead + self.nbytes].view(dtype)
        return out if shape is None else out.reshape(shape)


class Device:
    """The device flavour on guarded buffers: the mirror of tablebase_harness.Host."""

    def __init__(self, inventory):
        self.L, self.inventory, self.inv = nat.lib(), tuple(inventory), H.inv_array(inventory)
        self.aux = Guarded(nbytes=nat.TB_AUX_BYTES)
        self.stream = nat.current_stream(DEV)
        self._ok(self.L.gbl_tb_prepare(self.inv, self.aux.ptr, self.stream))
        self.positions = H.layout(inventory)[0]
        self.decided = torch.zeros(2, dtype=torch.int64, device=DEV)
        self.decided[1] = 0x5A5A

    def _ok(self, rc):
        assert rc == 0, self.L.gbl_last_error()

    def sweep(self, table_ptr, out_ptr, first, count, k):
        self._ok(self.L.gbl_tb_sweep(self.inv, self.aux.ptr, table_ptr, out_ptr, first, count, k, self.decided.data_ptr(), self.stream))

    def take_decided(self):
        both = self.decided.cpu().tolist()
        assert both[1] == 0x5A5A
        self.decided[0] = 0
        return both[0]


def device_build(dev, host_table_after, counts, slices=None):
    """Every sweep in place on the device, compared with the host flavour's table after that sweep (host_table_after(k)) and its count."""
    table = Guarded(nbytes=dev.positions)
    slices = slices or [(0, dev.positions)]
    for k, exp_count in enumerate(counts):
        for first, count in slices:
            dev.sweep(None if k == 0 else table.ptr, table.ptr + first, first, count, k)
        assert dev.take_decided() == exp_count, k
        assert np.array_equal(table.read(), host_table_after(k)), k
    return table


def host_sweeps(inventory):
    """The host flavour's build: (host, [table after sweep 0, 1, ...], counts)."""
    host = H.Host(inventory)
    table = np.zeros(host.positions, np.int8)
    after, counts, k = [], [], 0
    while True:
        counts.append(host.sweep(table, table, 0, host.positions, k))
        after.append(table.copy())
        if k > 0 and counts[-1] == 0:
            return host, after, counts
        k += 1


@pytest.fixture(scope="module")
def big(G):
    """(1, 1, 2) on the host, once: the final table, the counts, and the table after sweep k rebuilt from them (a byte is written once,
    in sweep |byte|)."""
    host = H.Host((1, 1, 2))
    table, counts = host.build()
    assert host.positions == 11783863 and len(counts) > 40
    mag = np.abs(table.astype(np.int16))
    return host, table, counts, lambda k: np.where((mag <= k) | (table == nat.TB_TERMINAL), table, 0).astype(np.int8)


def test_prepare_equals_the_host_flavour(G):
    dev = Device((2, 2, 2))
    assert np.array_equal(dev.aux.read(np.uint8), H.Host((2, 2, 2)).aux)


@pytest.mark.parametrize("inv", [(1, 1, 1), (2, 1, 0)])
def test_every_sweep_equals_the_host_flavour(G, inv):
    _, after, counts = host_sweeps(inv)
    device_build(Device(inv), lambda k: after[k], counts)


def test_every_sweep_of_a_large_universe_equals_the_host_flavour(G, big):
    host, table, counts, after = big
    device_build(Device((1, 1, 2)), after, counts)


def test_ragged_slices_and_a_buffer_of_its_own(G):
    host, after, counts = host_sweeps((2, 2, 0))
    dev = Device((2, 2, 0))
    table = device_build(dev, lambda k: after[k], counts[:8], H.ragged_slices(dev.positions))
    # sweep 8 of a slice into a buffer of its own beside the universe it reads, which stays as it was
    first, count = 12345, 70001
    part = Guarded(after[7][first:first + count], lead=1)   # (an odd address: bytes need no alignment)
    dev.sweep(table.ptr, part.ptr, first, count, 8)
    assert dev.take_decided() == int((np.abs(after[8][first:first + count].astype(np.int16)) == 8).sum())
    assert np.array_equal(part.read(), after[8][first:first + count]) and np.array_equal(table.read(), after[7])


def test_full_inventory_slices_equal_the_host_flavour(G):
    """Sweep 0 and sweep 1 with table = NULL on slices at 0, across 2^31 and at the end of the (2, 2, 2) universe."""
    host, dev = H.Host(H.FULL), Device(H.FULL)
    for first in H.FULL_SLICES:
        exp = np.full(H.SLICE, JUNK, np.int8)
        out = Guarded(nbytes=H.SLICE, lead=3)
        for k in (0, 1):
            count = host.sweep(None, exp, first, H.SLICE, k)
            dev.sweep(None, out.ptr, first, H.SLICE, k)
            assert dev.take_decided() == count and np.array_equal(out.read(), exp), (first, k)
        assert len(set(exp.tolist())) >= 2


def test_index_and_position_round_trips(G):
    host, dev = H.Host(H.FULL), Device(H.FULL)
    idx = np.array(H.FULL_SAMPLES + H.OUTSIDE + np.random.default_rng(12).integers(0, H.FULL_POSITIONS, 3000).tolist(), np.int64)
    n = len(idx)
    index_in, rows, back = Guarded(idx), Guarded(nbytes=27 * n, lead=1), Guarded(nbytes=8 * n)
    dev._ok(dev.L.gbl_tb_position(dev.inv, dev.aux.ptr, index_in.ptr, rows.ptr, n, dev.stream))
    to_move = torch.zeros(n, dtype=torch.int8, device=DEV)
    dev._ok(dev.L.gbl_tb_index(dev.inv, dev.aux.ptr, rows.ptr, to_move.data_ptr(), back.ptr, n, dev.stream))
    st = rows.read(np.int8, (n, 27))
    assert np.array_equal(st, host.position(idx))
    inside = (idx >= 0) & (idx < H.FULL_POSITIONS)
    assert np.array_equal(back.read(np.int64), np.where(inside, idx, -1)) and (~inside).sum() == len(H.OUTSIDE)
    # player_2 to move on the colour-swapped rows, and boards of a smaller inventory seen by either side
    small_host, small = H.Host((1, 2, 1)), Device((1, 2, 1))
    st, tm = H.sample_boards(small_host, 500, 13)
    st[7, 0] = 2  # a piece the inventory lacks
    rows, tmd, back = Guarded(st, lead=5), Guarded(tm, lead=3), Guarded(nbytes=8 * len(st))
    small._ok(small.L.gbl_tb_index(small.inv, small.aux.ptr, rows.ptr, tmd.ptr, back.ptr, len(st), small.stream))
    exp = small_host.index(st, tm)
    assert np.array_equal(back.read(np.int64), exp) and exp[7] == -1 and (np.delete(exp, 7) >= 0).all()


def device_probe(dev, table_ptr, st, tm, mask, keep=("outcome", "value", "action"), misaligned=False):
    n = len(st)
    bufs = {"state": Guarded(st, lead=1 * misaligned), "to_move": Guarded(tm, lead=3 * misaligned)}
    if mask is not None:
        bufs["mask"] = Guarded(mask, lead=5 * misaligned)
    outs = {"outcome": Guarded(nbytes=54 * n, lead=7 * misaligned), "value": Guarded(nbytes=n, lead=1 * misaligned),
            "action": Guarded(nbytes=4 * n, lead=4 * misaligned)}   # (action_out: 4-byte aligned at the least)
    dev._ok(dev.L.gbl_tb_probe(dev.inv, dev.aux.ptr, table_ptr, bufs["state"].ptr, bufs["to_move"].ptr, bufs["mask"].ptr if mask is not None else None,
                               *[outs[k].ptr if k in keep else None for k in outs], n, dev.stream))
    got = {"outcome": outs["outcome"].read(np.int8, (n, 54)), "value": outs["value"].read(np.int8), "action": outs["action"].read(np.int32)}
    for k in got:
        if k not in keep:
            assert (got[k].view(np.uint8) == JUNK).all(), k
    for k, a in (("state", st), ("to_move", tm)):
        assert np.array_equal(bufs[k].read(np.int8), np.ascontiguousarray(a).reshape(-1)), k
    return {k: v for k, v in got.items() if k in keep}


def test_probe_equals_the_host_flavour(G, big):
    host, table, counts, _ = big
    dev = Device((1, 1, 2))
    dtable = Guarded(table)
    st, tm = H.sample_boards(host, 1000, 14)
    mask = (np.random.default_rng(15).random((len(st), 54)) < 0.6).astype(np.int8)
    mask[11] = 0
    st[12, 0] = 2   # no state of the inventory
    for m, misaligned in ((None, False), (mask, False), (mask, True)):
        got, exp = device_probe(dev, dtable.ptr, st, tm, m, misaligned=misaligned), host.probe(table, st, tm, m)
        for k in exp:
            assert np.array_equal(got[k], exp[k]), (k, misaligned, np.argwhere(got[k] != exp[k])[:5])
    assert len(set(exp["value"].tolist())) > 8 and exp["action"][11] == -1 and exp["action"][12] == -1
    for keep in (("value",), ("action",), ("outcome",), ()):
        part = device_probe(dev, dtable.ptr, st, tm, mask, keep)
        assert all(np.array_equal(part[k], exp[k]) for k in keep)
    # a table of chosen bytes: every value a byte can hold, the widest results
    rng = np.random.default_rng(16)
    chosen = rng.integers(-126, 127, host.positions).astype(np.int8)
    chosen[rng.random(host.positions) < 0.1] = nat.TB_TERMINAL
    got, exp = device_probe(dev, Guarded(chosen).ptr, st, tm, mask), host.probe(chosen, st, tm, mask)
    assert all(np.array_equal(got[k], exp[k]) for k in exp) and {-127, 127} <= set(exp["outcome"].reshape(-1).tolist())


def test_a_probe_behind_the_last_sweep_needs_no_synchronisation(G):
    """Tablebase.build's sweeps and a probe on one stream, nothing in between; the class on the device against the class on the host."""
    inv = (2, 2, 0)
    cpu = G.Tablebase(inv, "cpu")
    counts = cpu.build()
    st, tm = H.sample_boards(H.Host(inv), 512, 17)
    tb = G.Tablebase(inv, DEV)
    tb.build(max_sweeps=len(counts) - 2)
    k = tb.sweeps
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        tb._decided.zero_()
        tb.sweep(k)                     # the last sweep that decides something ...
        got = tb.probe(st, tm)          # ... and the probe right behind it
        torch.cuda.current_stream().synchronize()
    assert int(tb._decided[0]) == counts[k] > 0
    exp = cpu.probe(st, tm)
    assert all(torch.equal(got[key].cpu(), exp[key]) for key in exp) and torch.equal(tb.table.cpu(), cpu.table)
    assert tb.build(slice_positions=300001) == counts[:k] + [0] and tb.complete   # (the device's own list lacks the sweep done by hand)
    env = G.BatchedGobblet(64, DEV)
    out = env.tablebase(tb)
    assert all(torch.equal(out[key].cpu(), cpu.probe(np.zeros((64, 27), np.int8), np.zeros(64, np.int8))[key]) for key in out)
