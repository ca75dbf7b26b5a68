"""Trajectory cells past 2^31 and 2^32 bytes on the MI355X (-m gpu): the self-play entry points take caller-given strides, and
strides_ok accepts any multiple of 16 that keeps the cells apart, so 130 boards x 3 plies reach such offsets in a few milliseconds.

One array at a time lives in ONE device buffer of 2^32 + 32 MiB canary bytes (never copied whole); every other trajectory output of the
call is NULL.  For a row of ROWB bytes the long stride is S = ((2^31 div ROWB) div 16) * 16 - 32 cells: time-major (ply_stride S,
tile_stride 64) puts ply 1 across 2^31 and ply 2 across 2^32; tile-major (ply_stride 64, tile_stride S) spreads tile 1 over 2^31 and
has tile 2 below 2^32 at ply 0 and above it at ply 2 -- asserted arithmetically before every launch.  The cells are gathered and
compared byte for byte with the host flavour's compact-stride window of the same call (a cell's content does not depend on the
strides), then overwritten with the canary on the device, after which the WHOLE buffer must be canary again: nothing outside the
cells, on either side of either boundary, is written.  The boards' final state, mover, done flag and turn equal the host's too.

Covered: the seven self-play entry points (gbl_collect_search, _eval, _solve, _noise, _cap, _gumbel, _tb) and gbl_collect_policy, every
trajectory array alone, both layouts; gbl_collect in each of its kernel forms at the form's smallest size, against the oracle (the
largest form takes 163 841 observation rows past 2^32: hence 32 MiB of slack, not a few KiB); the readers of a far window --
gbl_outcome_targets, gbl_training_batch, gbl_replay_append and gbl_replay_prio_append -- whose arrays share the call's one stride, so
that the widest required array passes 2^32 and each narrower one goes as far as its rows take it (printed per array); and
gbl_reanalyse and gbl_tb_targets on rows 2^30 + 128 bytes apart, one array at a time."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle

from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as ER
from tests import selfplay_harness as H
from tests import selfplay_tb_harness as HT
from tests import symmetry_restatement as S
from tests import tablebase_harness as TH
from tests.gumbel_harness import device_collect_gumbel, host_collect_gumbel
from tests.search_harness import DEV, G  # noqa: F401  (G: the fixture)
from tests.selfplay_cap_harness import device_collect_cap, host_collect_cap
from tests.selfplay_harness import DeviceNet, geometry
from tests.test_selfplay_solve import fixture_boards, smoke_net

pytestmark = pytest.mark.gpu

CANARY = 0xA5
FAR_BYTES = (1 << 32) + (32 << 20)  # (gbl_collect's largest form takes 163 841 rows of 117 bytes past 2^32)
N, T = 130, 3
X, SAMPLE_PLIES, SEED, ENV_BASE, PLY0 = 48, 2, 0xFEDCBA9876543210, (1 << 41) + 77, 3
INVENTORY = (1, 1, 0)


class Far:
    """The far buffer as a store of the harness runners (tests/selfplay_harness.py::Compact's two methods): the one array of the call
    starts at byte 0; cells() gathers, restores the canary in the cells and requires the whole buffer to be canary again."""

    def __init__(self):
        self.raw = torch.full((FAR_BYTES,), CANARY, dtype=torch.uint8, device=DEV)
        self.words = self.raw.view(torch.int64)
        self.word = int(np.full(8, CANARY, np.uint8).view(np.int64)[0])
        self.views = {}

    def array(self, k, dt, tail, total, offset=0):
        """Array k of `total` rows from byte `offset` of the buffer (the self-play runners give one array per call, at byte 0; a call
        whose arrays share one stride keeps them apart by their offsets)."""
        dt = np.dtype(dt)
        nbytes = total * int(np.prod(tail, dtype=np.int64)) * dt.itemsize
        assert offset % 16 == 0 and offset + nbytes <= FAR_BYTES
        fill = int(np.full(dt.itemsize, CANARY, np.uint8).view(dt)[0])
        self.views[k] = self.raw[offset:offset + nbytes].view(getattr(torch, dt.name)).view((total,) + tuple(tail)), fill
        return self.views[k][0]

    def put(self, k, at, values):
        """An input array's cells, from the host: one plain copy per run of consecutive cells (a slice checks its bounds on the host)."""
        view = self.views[k][0]
        flat = np.ascontiguousarray(at).ravel()
        rows = torch.from_numpy(np.ascontiguousarray(values).reshape((-1,) + tuple(view.shape[1:]))).to(DEV)
        cuts = np.flatnonzero(np.diff(flat) != 1) + 1
        for lo, hi in zip(np.r_[0, cuts], np.r_[cuts, len(flat)]):
            view[int(flat[lo]):int(flat[lo]) + int(hi - lo)].copy_(rows[int(lo):int(hi)])

    def dirty(self):
        """How many 8-byte words of the buffer are not canary, counted 256 MiB at a time (the comparison's temporary stays small)."""
        return int(sum(torch.count_nonzero(part != self.word) for part in self.words.split(1 << 25)))

    def cells(self, at, total=None):
        """{k: the cells of array k on the host}; the cells are canary again afterwards, and so must the whole buffer be."""
        idx = torch.from_numpy(np.ascontiguousarray(at).ravel()).to(DEV)
        got = {}
        for k, (view, fill) in self.views.items():
            got[k] = view[idx].cpu().numpy().reshape(at.shape + tuple(view.shape[1:]))
            view[idx] = fill
        self.views = {}
        dirty = self.dirty()
        if dirty:  # (the next case starts clean whatever this one did)
            self.raw.fill_(CANARY)
        assert dirty == 0, "%s: %d words outside the cells were written" % (sorted(got), dirty)
        return got


@pytest.fixture(scope="module")
def far(G):
    """An allocation that fails fails the test."""
    torch.cuda.empty_cache()
    buf = Far()
    yield buf
    del buf.raw, buf.words, buf.views
    torch.cuda.empty_cache()


def far_strides(rowb, layout):
    S = ((2 ** 31 // rowb) // 16) * 16 - 32
    return (S, 64) if layout == "time" else (64, S)


def reach(rowb, layout, n=N, plies=T):
    """The largest byte offset the array's cells reach under far_strides, after asserting where they lie about 2^31 and 2^32 (so that a
    later change of n or T cannot quietly move everything below a boundary)."""
    _, _, total, at = geometry(n, plies, layout, far_strides(rowb, layout))
    first, last = at.astype(np.int64) * rowb, at.astype(np.int64) * rowb + rowb - 1
    assert total * rowb <= FAR_BYTES and last.max() == total * rowb - 1 - (63 - (n - 1) % 64) * rowb
    if layout == "time":  # ply 1 straddles 2^31, ply 2 straddles 2^32: the first board past either lies inside the ply
        for t, edge, lo, hi in ((1, 1 << 31, 32, 44), (2, 1 << 32, 64, 88)):
            past = first[t] >= edge
            assert first[t, 0] < edge and lo <= int(np.argmax(past)) <= hi, (rowb, t, int(np.argmax(past)))
        assert last[0].max() < 1 << 31
    else:  # tile 1 is spread over 2^31; tile 2 is below 2^32 at ply 0 and above it at ply 2
        assert first[:, 64:128].min() < 1 << 31 <= first[:, 64:128].max() and last[:, :64].max() < 1 << 31
        assert last[0, 128:].max() < 1 << 32 <= first[2, 128:].min()
    assert ((first >= 1 << 31) & (last < 1 << 32)).any() and (first >= 1 << 32).any()
    return int(last.max())


@pytest.mark.parametrize("layout", ["time", "tile"])
@pytest.mark.parametrize("rowb", [1, 2, 4, 54, 108, 117])
def test_the_geometry_straddles_both_boundaries(rowb, layout):
    assert 1 << 32 <= reach(rowb, layout) < FAR_BYTES


# ---- the self-play family ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boards(G):
    """Boards 0 .. 39 empty, then the midgame fixture, some inside the sampled plies."""
    st, tm, turn = fixture_boards(N - 40, DEV)
    return (np.ascontiguousarray(np.concatenate([np.zeros((40, 27), np.int8), st])), np.concatenate([np.zeros(40, np.int8), tm]),
            np.concatenate([np.zeros(40, np.int32), turn % 4]).astype(np.int32))


@pytest.fixture(scope="module")
def nets(G):
    """(host nets, device nets): H = 64 against 128."""
    pair = (smoke_net(), ER.random_net(128, 77))
    return pair, tuple(DeviceNet(x) for x in pair)


@pytest.fixture(scope="module")
def table(G):
    """The (1, 1, 0) table built on the device: (device Table, host Table, 130 start boards of the three kinds)."""
    tb = G.Tablebase(INVENTORY, DEV)
    tb.build()
    assert tb.complete
    host = TH.Host(INVENTORY)
    assert np.array_equal(tb._aux.cpu().numpy(), host.aux)
    st, tm, turn = HT.start_boards(host, 120, 40, 20, seed=71)  # (the sampler returns the quiet positions among those asked for)
    pick = np.r_[0:N - 60, len(st) - 60:len(st)]
    assert len(st) >= N and len(pick) == N
    return (HT.Table(INVENTORY, tb._aux, tb.table), HT.Table(INVENTORY, host.aux, tb.table.cpu().numpy()),
            (np.ascontiguousarray(st[pick]), np.ascontiguousarray(tm[pick]), np.ascontiguousarray(turn[pick])))


def plain(entry, **sides):
    """gbl_collect_search / _eval / _solve / _noise: (names, device runner, host runner) over (boards, nets of the flavour, layout)."""
    name = "gbl_cpu_collect_search" + ("" if entry == "search" else "_" + entry)
    pols = ("tree", "tree") if entry == "search" else ("eval", "eval")

    def dev(b, dn, layout, **kw):
        return H.device_collect(entry, *b, T, pols, X, SAMPLE_PLIES, nat.ILLEGAL_NOOP, layout, SEED, ENV_BASE, PLY0,
                                **({} if entry == "search" else {"nets": dn}), **sides, **kw)

    def host(b, hn, layout):
        L = nat.cpu_raw()
        return H.host_collect(entry, getattr(L, name), L.gbl_cpu_last_error, *b, T, pols, X, SAMPLE_PLIES, nat.ILLEGAL_NOOP, layout, SEED,
                              ENV_BASE, PLY0, **({} if entry == "search" else {"nets": hn}), **sides)
    return H.NAMES[entry], dev, host


COMMON = dict(X=X, sample_plies=SAMPLE_PLIES, seed=SEED, env_base=ENV_BASE, ply0=PLY0)
CAP = dict(its=(8, 8), fast=(3, 3), share=(128, 64), deps=(2, 2), noise=(64, 0), **COMMON)
GUMBEL = dict(its=(8, 8), considered=(16, 4), **COMMON)
FAMILY = {  # eight iterations where a search runs, depth 2 for the solver
    "search": plain("search", its=(8, 8), pls=(2, 2), M=20),
    "eval": plain("eval", its=(8, 8)),
    "solve": plain("solve", its=(8, 8), deps=(2, 2)),
    "noise": plain("noise", its=(8, 8), deps=(2, 0), noise=(64, 32)),
    "cap": (H.SOLVE_NAMES, lambda b, dn, layout, **kw: device_collect_cap(*b, T, ("eval", "eval"), dn, layout=layout, **CAP, **kw),
            lambda b, hn, layout: host_collect_cap(*b, T, ("eval", "eval"), hn, layout=layout, **CAP)),
    "gumbel": (H.EVAL_NAMES, lambda b, dn, layout, **kw: device_collect_gumbel(*b, T, ("eval", "eval"), dn, layout=layout, **GUMBEL, **kw),
               lambda b, hn, layout: host_collect_gumbel(*b, T, ("eval", "eval"), hn, layout=layout, **GUMBEL)),
}
TB = dict(its=(8, 0), deps=(2, 0), noise=(64, 0), mode=1, count=2, **COMMON)


def sweep(far, names, dev, exp, layout, what):
    """Every array of `names` alone under its far geometry against the compact window `exp` of the host flavour."""
    for k, dt, tail in names:
        rowb = int(np.prod(tail, dtype=np.int64)) * np.dtype(dt).itemsize
        assert exp[0][k].shape[:2] == (T, N)
        top = reach(rowb, layout)
        got = dev(keep=[k], strides=far_strides(rowb, layout), store=far)
        assert list(got[0]) == [k] and got[0][k].dtype == exp[0][k].dtype
        assert np.array_equal(got[0][k], exp[0][k]), (what, k, layout, np.argwhere(got[0][k] != exp[0][k])[:5])
        for name, g, e in zip(("state", "to_move", "done", "turn"), got[1:], exp[1:]):
            assert np.array_equal(g, e), (what, k, layout, name)
        print("%s %s %s: row of %d bytes, largest byte offset written %d = 2^32 + %d" % (what, layout, k, rowb, top, top - (1 << 32)))


@pytest.mark.parametrize("layout", ["time", "tile"])
@pytest.mark.parametrize("entry", sorted(FAMILY))
def test_selfplay_cells_past_32_bits(G, far, boards, nets, entry, layout):
    names, dev, host = FAMILY[entry]
    hn, dn = nets
    exp = host(boards, hn, layout)
    assert {0, 1} == set(np.unique(exp[0]["mover"]).tolist()) and (exp[0]["visits"] != 0).any()
    sweep(far, names, lambda **kw: dev(boards, dn, layout, **kw), exp, layout, "gbl_collect_search" + ("" if entry == "search" else "_" + entry))


@pytest.mark.parametrize("layout", ["time", "tile"])
def test_selfplay_tb_cells_past_32_bits(G, far, table, nets, layout):
    """... and the table's three judge trajectories beside the rest: the evaluator against the (1, 1, 0) table."""
    dev_tb, host_tb, b = table
    hn, dn = nets
    exp = HT.host_collect_tb(host_tb, *b, T, ("eval", "tb"), (hn[0], None), layout=layout, **TB)
    assert np.isin(exp[0]["how"], (nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED)).any() and (exp[0]["how"] == nat.HOW_SEARCH).any()
    sweep(far, HT.TB_NAMES, lambda **kw: HT.device_collect_tb(dev_tb, *b, T, ("eval", "tb"), (dn[0], None), layout=layout, **TB, **kw), exp,
          layout, "gbl_collect_search_tb")


# ---- gbl_collect: every kernel form at its smallest size ------------------------------------------------------------------------------------------
COLLECT_NAMES = H.SCALARS[:7]  # actions, winner, rewards, done, to_move, action_mask, observation: gbl_collect's seven, in ABI order
WARM, COLLECT_SEED, COLLECT_BASE = 6, 29, 123_456_789_012
# (kernel form, boards, the variant gbl_collect_variant reports WITH the arrays the case gives, the layouts whose cells fit the buffer:
# tile-major takes a tile stride of S, so only three tiles fit)
ROLES = 1000  # GBL_COLLECT_IS_ROLES: k_collect_small
FORMS = [("k_collect5", 130, 5, ("time", "tile")), ("k_collect_small", 130, ROLES, ("time", "tile")), ("k_collect3", 9217, 4, ("time",)),
         ("k_collect2", 45057, 2, ("time",)), ("k_collect", 163841, 0, ("time",))]


def oracle_window(n):
    """(start arrays, {name: (T, n, ...)} of the oracle's fused plies WARM .. WARM + T - 1, final arrays) of n boards from reset."""
    s, tm, dn = oracle.batch_reset(n)
    oracle.batch_rollout(s, tm, dn, COLLECT_SEED, COLLECT_BASE, 0, WARM, threads=16, want_obs=False, want_mask=False)
    start, plies = (s.copy(), tm.copy(), dn.copy()), []
    for t in range(T):
        o = oracle.batch_rollout(s, tm, dn, COLLECT_SEED, COLLECT_BASE, WARM + t, 1, threads=16)
        plies.append(dict(actions=o["actions"], winner=o["winner"], rewards=o["reward"], done=dn.copy(), to_move=tm.copy(),
                          action_mask=o["mask"], observation=o["obs"].reshape(n, 117)))
    return start, {k: np.stack([p[k] for p in plies]) for k in plies[0]}, (s, tm, dn)


def collect_far(far, window, n, layout, under_test, beside=()):
    """gbl_collect with the array `under_test` in the far buffer under its own far strides, the arrays named in `beside` in compact
    memory of their own under the same strides (they reach as far as their narrower rows take them), every other trajectory NULL.
    Returns the largest byte offset of the far array and of each array beside it."""
    start, exp, final = window
    table = {k: (np.dtype(dt), tail) for k, dt, tail in COLLECT_NAMES}
    rowb = lambda k: int(np.prod(table[k][1], dtype=np.int64)) * table[k][0].itemsize  # noqa: E731
    ps, ts = far_strides(rowb(under_test), layout)
    tops = {under_test: reach(rowb(under_test), layout, n)}
    _, _, total, at = geometry(n, T, layout, (ps, ts))
    given = {under_test: far.array(under_test, *table[under_test], total)}
    for k in beside:
        assert rowb(k) < rowb(under_test)
        given[k] = torch.full((total,) + table[k][1], -7, dtype=getattr(torch, table[k][0].name), device=DEV)
        tops[k] = int(at.max() + 1) * rowb(k) - 1
    st, tm, dn = (torch.from_numpy(x).to(DEV) for x in start)
    nat.check(nat.lib().gbl_collect(nat.ptr(st), nat.ptr(tm), nat.ptr(dn), *[nat.ptr(given.get(k)) for k, _, _ in COLLECT_NAMES], n, ps, ts,
                                    COLLECT_SEED, COLLECT_BASE, WARM, None, T, nat.ILLEGAL_NOOP, None, None, nat.current_stream(DEV)),
              "gbl_collect")
    torch.cuda.synchronize()
    idx = torch.from_numpy(at.ravel()).to(DEV)
    for k in beside:
        got = given[k][idx].cpu().numpy().reshape(exp[k].shape)
        assert np.array_equal(got, exp[k]), (k, "beside", under_test)
        given[k][idx] = -7
        assert bool((given[k] == -7).all()), "output %s was written outside its cells" % k
    got = far.cells(at, total)[under_test]
    assert got.dtype == exp[under_test].dtype and np.array_equal(got, exp[under_test]), (under_test, np.argwhere(got != exp[under_test])[:5])
    for name, mine, ref in zip(("state", "to_move", "done"), (st, tm, dn), final):
        assert np.array_equal(mine.cpu().numpy(), ref), name
    return tops


@pytest.mark.parametrize("form,n,variant,layouts", FORMS, ids=[f[0] for f in FORMS])
def test_collect_cells_past_32_bits(G, far, form, n, variant, layouts):
    """The reference is the oracle's fused ply, as tests/test_gpu_bench_kernels.py::check_trajectory takes it.  A form that needs the
    mask trajectory runs FULL with the observation rows far and the mask rows beside them under the same strides (54 / 117 of the way:
    below 2^31), and MASK_ONLY with the mask rows far and the five scalar arrays beside them under the mask's strides.  So the scalars
    of k_collect5, k_collect3, k_collect2 and k_collect are never far themselves -- at most 4 / 54 of the way, below 2^29 bytes --
    because those forms exist only with a mask trajectory, whose stride they share; k_collect_small (no mask trajectory) takes the
    observation rows alone, and every scalar array alone and far."""
    L = nat.lib()
    window = oracle_window(n)
    assert window[1]["done"].any() or n < 1000  # (games end inside the window of the larger launches)
    for layout in layouts:
        if variant == ROLES:
            assert L.gbl_collect_variant(n, T, 0, 1) >= ROLES
            cases = [("observation", ())] + [(k, ()) for k, _, _ in COLLECT_NAMES[:5]]
        else:
            assert L.gbl_collect_variant(n, T, 1, 1) == variant
            cases = [("observation", ("action_mask",)), ("action_mask", tuple(k for k, _, _ in COLLECT_NAMES[:5]))]
        for under_test, beside in cases:
            tops = collect_far(far, window, n, layout, under_test, beside)
            for k, top in tops.items():
                print("gbl_collect %s %s %s%s: largest byte offset written %d = 2^32 %+d" % (
                    form, layout, k, " (beside %s)" % under_test if k != under_test else "", top, top - (1 << 32)))


# ---- several arrays of one launch in the far buffer ------------------------------------------------------------------------------------------------
def place(far, names, at, total):
    """The arrays `names` = (name, dtype, row tail, byte offset in the buffer) of one launch in the far buffer under the launch's one
    stride: ({name: view}, {name: the array's largest byte offset}).  No two cells of any of them may meet."""
    views, tops, spans = {}, {}, []
    for k, dt, tail, offset in names:
        rowb = int(np.prod(tail, dtype=np.int64)) * np.dtype(dt).itemsize
        views[k] = far.array(k, dt, tail, total, offset)
        first = offset + at.ravel().astype(np.int64) * rowb
        spans += [(int(f), int(f) + rowb) for f in first]
        tops[k] = int(first.max()) + rowb - 1
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "cells of two arrays meet"
    return views, tops


def report(what, tops, written=()):
    for k, top in tops.items():
        edge, name = (1 << 32, "2^32") if top >= 1 << 32 else (1 << 31, "2^31")
        print("%s %s (%s): largest byte offset %d = %s %+d" % (what, k, "written" if k in written else "read", top, name, top - edge))


# ---- gbl_outcome_targets: a far-strided window read and written ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["time", "tile"])
def test_outcome_targets_on_a_far_window(G, far, layout):
    """The five arrays share the call's one stride: S is that of the two-byte rows (reward read, plies_left written: past 2^32), the
    one-byte arrays (done and mover read, z written) go half as far (past 2^31).  All five live in the far buffer, kept apart by their
    byte offsets (place); the window is a synthetic one with game ends in it, the reference the host flavour on compact strides."""
    from tests.test_selfplay_search import targets
    rng = np.random.default_rng(31)
    done = (rng.random((T, N)) < 0.3).astype(np.int8)
    rewards = rng.choice(np.array([-1, 0, 1], np.int8), (T, N, 2))
    mover = rng.integers(0, 2, (T, N)).astype(np.int8)
    z, left = targets(nat.cpu_raw(), done, rewards, mover, layout)
    assert (z == nat.Z_OPEN).any() and (z != nat.Z_OPEN).any() and (left > 0).any()
    ps, ts = far_strides(2, layout)
    reach(2, layout)
    _, _, total, at = geometry(N, T, layout, (ps, ts))
    v, tops = place(far, (("rewards", np.int8, (2,), 0), ("left", np.int16, (), 1024), ("done", np.int8, (), 2048), ("mover", np.int8, (), 2560),
                          ("z", np.int8, (), 3072)), at, total)
    for k, a in (("rewards", rewards), ("done", done), ("mover", mover)):
        far.put(k, at, a)
    nat.check(nat.lib().gbl_outcome_targets(nat.ptr(v["done"]), nat.ptr(v["rewards"]), nat.ptr(v["mover"]), nat.ptr(v["z"]), nat.ptr(v["left"]),
                                            N, ps, ts, T, nat.current_stream(DEV)), "gbl_outcome_targets")
    torch.cuda.synchronize()
    got = far.cells(at)
    assert np.array_equal(got["z"], z) and np.array_equal(got["left"], left)
    assert np.array_equal(got["rewards"], rewards) and np.array_equal(got["done"], done) and np.array_equal(got["mover"], mover)
    assert all(tops[k] >= 1 << 32 for k in ("rewards", "left")) and all(1 << 31 <= tops[k] < 1 << 32 for k in ("done", "mover", "z"))
    report("gbl_outcome_targets " + layout, tops, written=("z", "left"))


# ---- pitched rows: gbl_reanalyse and gbl_tb_targets -----------------------------------------------------------------------------------------------------------------------
PITCH_BYTES = (1 << 30) + 128  # rows 2 and 4 start past 2^31 and 2^32


def pitched(far, src, name, twins=None):
    """The pitched arrays of one call: src = {k: (rows (n, row), the ring's pitch in elements)}.  Array `name` lies in the far buffer, a
    flat array whose row r starts at element r * (PITCH_BYTES / itemsize); twins = {k: output name} puts an output array of the same
    pitch 1 024 bytes further on (not in place).  Every other array lies at its ring pitch in compact memory, junk in the padding.
    Returns ({k: pointer}, {k: pitch in elements}, the far array's element indices (n, row), the tensors to keep alive)."""
    n = len(src[name][0])
    assert 2 * PITCH_BYTES >= 1 << 31 and 4 * PITCH_BYTES >= 1 << 32 and 4 * PITCH_BYTES + 2048 <= FAR_BYTES
    ptr, pitch, hold, where = {}, {}, [], None
    for k, (a, ring_pitch) in src.items():
        a = np.ascontiguousarray(a)
        row = a.shape[1]
        if k == name:
            pitch[k] = PITCH_BYTES // a.dtype.itemsize
            where = np.arange(n)[:, None] * pitch[k] + np.arange(row)
            ptr[k] = nat.ptr(far.array(k, a.dtype, (), (n - 1) * pitch[k] + 128))
            far.put(k, where, a)
            if twins and k in twins:
                ptr[twins[k]] = nat.ptr(far.array(twins[k], a.dtype, (), (n - 1) * pitch[k] + 128, 1024))
        else:
            t = torch.full((n, ring_pitch), 0x5A, dtype=getattr(torch, a.dtype.name), device=DEV)
            t[:, :row] = torch.from_numpy(a).to(DEV)
            hold.append(t)
            pitch[k], ptr[k] = ring_pitch, nat.ptr(t)
    return ptr, pitch, where, hold


@pytest.fixture(scope="module")
def five_rows(G):
    """Five rows of tests/reanalyse_harness.py::make_rows: four that are searched again and one that is skipped (z = GBL_Z_OPEN), and the
    host flavour's results on them at the ring's pitches, in place and not."""
    from tests import reanalyse_harness as RH
    from tests.tb_targets_harness import RING
    net = RH.net64()
    obs, mask, vis, z = RH.make_rows(net)
    pick = np.concatenate([np.flatnonzero(z != nat.Z_OPEN)[[0, 1, -2, -1]], np.flatnonzero(z == nat.Z_OPEN)[:1]])[[0, 1, 4, 2, 3]]
    rows = tuple(np.ascontiguousarray(x[pick]) for x in (obs, mask, vis, z))
    exp = {inplace: RH.run(RH.Env(net), *rows, layout=RING, inplace=inplace) for inplace in (True, False)}
    return net, rows, exp


@pytest.mark.parametrize("which", ["obs", "mask", "visits_inplace", "visits", "z"])
def test_reanalyse_rows_at_a_far_pitch(G, far, five_rows, which):
    """n = 5 rows 2^30 + 128 bytes apart in the far buffer for ONE array, the others at their ring pitches in compact memory."""
    from tests import reanalyse_harness as RH
    net, (obs, mask, vis, z), exp = five_rows
    n, inplace = 5, which != "visits"
    src = {"obs": (obs, nat.REPLAY_OBS_PITCH), "mask": (mask, nat.REPLAY_META_PITCH), "visits": (vis, nat.REPLAY_VISITS_PITCH),
           "z": (z.reshape(n, 1), nat.REPLAY_META_PITCH)}
    name = which.split("_")[0]
    ptr, pitch, where, _hold = pitched(far, src, name, {"visits": "visits_out"} if which == "visits" else {})
    if "visits_out" not in ptr:
        ptr["visits_out"] = ptr["visits"]
    dense = {k: torch.full((n, row), 0x5A, dtype=getattr(torch, np.dtype(dt).name), device=DEV) for k, dt, row in RH.DENSE}
    dev = RH.Env(net, DEV)
    ev = net.struct(dev.arrays)
    nat.check(nat.lib().gbl_reanalyse(C.addressof(ev), 8, RH.EXPLORE, ptr["obs"], pitch["obs"], ptr["mask"], pitch["mask"], ptr["visits"],
                                      ptr["visits_out"], pitch["visits"], ptr["z"], pitch["z"], *[nat.ptr(dense[k]) for k in RH.ALL], n,
                                      dev.stream), "gbl_reanalyse")
    torch.cuda.synchronize()
    e = exp[inplace]
    for k, dt, row in RH.DENSE:
        got = dense[k].cpu().numpy()
        assert np.array_equal(got if row > 1 else got[:, 0], e[k]), (which, k)
    assert (e["census"] != e["census"][2]).any()  # (searched rows and the skipped one)
    if name == "visits":
        cells = far.cells(where)
        new = cells["visits_out"] if which == "visits" else cells["visits"]
        if which == "visits":
            assert np.array_equal(cells["visits"], vis), "visits_in was written"
            searched = (e["visits"] != np.int16(0x5A5A)).any(1)  # (the host's not-in-place output rows start as the same junk)
            junk = int(np.full(2, CANARY, np.uint8).view(np.int16)[0])
            assert np.array_equal(new[searched], e["visits"][searched]) and (new[~searched] == junk).all() and searched.sum() == 4
        else:
            assert np.array_equal(new, e["visits"])
    else:
        cells = far.cells(where)
        assert np.array_equal(cells[name], src[name][0]), "an input row was written"
    print("gbl_reanalyse %s: rows at byte %s, the last past 2^32 by %d" % (which, [r * PITCH_BYTES for r in range(n)], 4 * PITCH_BYTES - (1 << 32)))


@pytest.fixture(scope="module")
def tb_rows(G, table):
    """Five rows of the (1, 1, 0) table's positions with old targets, the middle one skipped (z = GBL_Z_OPEN); the device and host
    environments of tests/tb_targets_harness.py on the built table, and the host flavour's results at the ring's pitches."""
    from tests import tb_targets_harness as TT
    from tests.test_gpu_tb_targets import DevEnv
    dev_tb, host_tb, _ = table
    henv, denv = TT.HostEnv(INVENTORY, host_tb.table), DevEnv(INVENTORY, dev_tb.table)
    obs, st, tm = TT.position_rows(henv.host, 40, 5)
    mask = TT.legal_mask(st, tm)
    v_old, z_old = TT.old_targets(len(obs), 50)
    labelled = TT.run(henv, obs, mask, v_old, z_old, 1, 600, layout=TT.RING, inplace=False)["z"] != TT.JUNK
    pick = np.concatenate([np.flatnonzero(labelled)[[0, 1, -2, -1]], np.flatnonzero(z_old == nat.Z_OPEN)[:1]])[[0, 1, 4, 2, 3]]
    rows = tuple(np.ascontiguousarray(x[pick]) for x in (obs, mask, v_old, z_old))
    exp = {inplace: TT.run(henv, *rows, 1, 600, layout=TT.RING, inplace=inplace) for inplace in (True, False)}
    assert (exp[False]["z"] != TT.JUNK).sum() == 4 and exp[False]["z"][2] == TT.JUNK
    return denv, rows, exp


@pytest.mark.parametrize("which", ["obs", "mask", "visits_inplace", "visits", "z_inplace", "z"])
def test_tb_targets_rows_at_a_far_pitch(G, far, tb_rows, which):
    """gbl_tb_targets the same way: mode "shortest", count 600; visits and z in place and not (the outputs share their input's pitch)."""
    from tests import tb_targets_harness as TT
    denv, (obs, mask, vis, z), exp = tb_rows
    n, name = 5, which.split("_")[0]
    inplace = which not in ("visits", "z")
    src = {"obs": (obs, nat.REPLAY_OBS_PITCH), "mask": (mask, nat.REPLAY_META_PITCH), "visits": (vis, nat.REPLAY_VISITS_PITCH),
           "z": (z.reshape(n, 1), nat.REPLAY_META_PITCH)}
    ptr, pitch, where, hold = pitched(far, src, name, {} if inplace else {name: name + "_out"})
    compact = {}  # the output rows that are not far: in place the inputs' own, else junk rows at the ring's pitch
    for k, dt, junk in (("visits", torch.int16, 0x5A5A), ("z", torch.int8, TT.JUNK)):
        if k + "_out" not in ptr:
            if inplace:
                ptr[k + "_out"] = ptr[k]
                compact[k] = None if k == name else hold[[x for x in src if x != name].index(k)]
            else:
                compact[k] = torch.full((n, pitch[k]), junk, dtype=dt, device=DEV)
                ptr[k + "_out"] = nat.ptr(compact[k])
    dense = {"value": torch.full((n,), TT.JUNK, dtype=torch.int8, device=DEV), "outcome": torch.full((n, 54), TT.JUNK, dtype=torch.int8, device=DEV),
             "census": torch.full((n,), TT.JUNK, dtype=torch.int8, device=DEV)}
    rc = denv.L.gbl_tb_targets(denv.inv, denv.aux_ptr, denv.table_ptr, ptr["obs"], pitch["obs"], ptr["mask"], pitch["mask"], ptr["visits"],
                               ptr["visits_out"], pitch["visits"], ptr["z"], ptr["z_out"], pitch["z"], 1, 600,
                               *[nat.ptr(dense[k]) for k in ("value", "outcome", "census")], n, denv.stream)
    assert rc == 0, denv.error()
    torch.cuda.synchronize()
    e = exp[inplace]
    for k, t in dense.items():
        assert np.array_equal(t.cpu().numpy(), e[k]), (which, k)
    cells = far.cells(where)
    written = exp[False]["z"] != TT.JUNK  # (a row that is skipped keeps what its output row held: the input in place, junk or canary otherwise)
    for k, row, host_junk in (("visits", 54, 0x5A5A), ("z", 1, TT.JUNK)):
        if k == name:
            new = cells[k] if inplace else cells[k + "_out"]
            if not inplace:
                assert np.array_equal(cells[k], src[k][0]), "an input row was written"
                canary = int(np.full(new.dtype.itemsize, CANARY, np.uint8).view(new.dtype)[0])
                assert (new[~written] == canary).all()
        else:
            new = compact[k].cpu().numpy()[:, :row]
            assert inplace or (new[~written] == host_junk).all()
        ref = e[k].reshape(n, row)
        assert np.array_equal(new[written], ref[written]) and (inplace is False or np.array_equal(new, ref)), (which, k)
    if name in ("obs", "mask"):
        assert np.array_equal(cells[name], src[name][0]), "an input row was written"
    print("gbl_tb_targets %s: rows at byte %s, the last past 2^32 by %d" % (which, [r * PITCH_BYTES for r in range(n)], 4 * PITCH_BYTES - (1 << 32)))


# ---- gbl_collect_policy --------------------------------------------------------------------------------------------------------------------------------
POLICY_NAMES = COLLECT_NAMES + (("chosen", np.int32, ()), ("how", np.int8, ()), ("candidates", np.int8, (54,)))
POLICIES, OPENING = (2, 0), 1  # greedy at depth 2 against masked-random, one random opening ply


@pytest.fixture(scope="module")
def policy_window(G):
    """As tests/test_gpu_policy_collect.py::run_and_check: 130 boards after six masked-random plies, histories that matter from the
    first ply on, and the oracle's three policy plies.  (start arrays, {name: (T, n, ...)}, final arrays.)"""
    s, tm, dn = oracle.batch_reset(N)
    turn = np.zeros(N, np.int32)
    oracle.batch_rollout(s, tm, dn, COLLECT_SEED, COLLECT_BASE, 0, WARM, threads=16, want_obs=False, want_mask=False, turn=turn)
    hist = np.random.default_rng(5).integers(-1, 54, (N, 2, 3)).astype(np.int8)
    start, plies = tuple(x.copy() for x in (s, tm, dn, hist, turn)), []
    for t in range(T):
        o = oracle.batch_policy_ply(s, tm, dn, hist, turn, COLLECT_SEED, COLLECT_BASE, WARM + t, POLICIES, OPENING, illegal_mode=0, threads=16)
        plies.append(dict(actions=o["actions"], winner=o["winner"], rewards=o["reward"], done=dn.copy(), to_move=tm.copy(),
                          action_mask=o["mask"], observation=o["obs"].reshape(N, 117), chosen=o["chosen"], how=o["how"], candidates=o["cands"]))
    exp = {k: np.stack([p[k] for p in plies]) for k in plies[0]}
    assert {0, 1, 2} <= set(np.unique(exp["how"]).tolist()) and (exp["candidates"] != 0).any()  # random, greedy and fallback plies
    return start, exp, (s, tm, dn, hist, turn)


@pytest.mark.parametrize("layout", ["time", "tile"])
def test_policy_collect_cells_past_32_bits(G, far, policy_window, layout):
    """Every one of gbl_collect_policy's ten trajectory arrays alone under its far geometry (each may be NULL), against the oracle."""
    start, exp, final = policy_window
    for k, dt, tail in POLICY_NAMES:
        rowb = int(np.prod(tail, dtype=np.int64)) * np.dtype(dt).itemsize
        top = reach(rowb, layout)
        ps, ts = far_strides(rowb, layout)
        _, _, total, at = geometry(N, T, layout, (ps, ts))
        given = {k: far.array(k, dt, tail, total)}
        st, tm, dn, hist, turn = (torch.from_numpy(x).to(DEV) for x in start)
        nat.check(nat.lib().gbl_collect_policy(nat.ptr(st), nat.ptr(tm), nat.ptr(dn), nat.ptr(hist), *[nat.ptr(given.get(x)) for x, _, _ in POLICY_NAMES],
                                               N, ps, ts, COLLECT_SEED, COLLECT_BASE, WARM, None, T, POLICIES[0], POLICIES[1], OPENING,
                                               nat.ILLEGAL_NOOP, None, nat.ptr(turn), nat.current_stream(DEV)), "gbl_collect_policy")
        torch.cuda.synchronize()
        got = far.cells(at, total)[k]
        assert got.dtype == np.dtype(dt) and np.array_equal(got, exp[k]), (k, layout, np.argwhere(got != exp[k])[:5])
        for name, mine, ref in zip(("state", "to_move", "done", "hist", "turn"), (st, tm, dn, hist, turn), final):
            assert np.array_equal(mine.cpu().numpy(), ref), (k, name)
        print("gbl_collect_policy %s %s: row of %d bytes, largest byte offset written %d = 2^32 %+d" % (layout, k, rowb, top, top - (1 << 32)))


# ---- readers of a far-strided window: gbl_training_batch and the two replay appends --------------------------------------------------------------------
WINDOW_NAMES = (("obs", np.int8, (117,)), ("visits", np.int16, (54,)), ("mask", np.int8, (54,)), ("z", np.int8, ()), ("done", np.int8, ()),
                ("mover", np.int8, ()), ("prio", np.int32, ()))


def far_window(far, w, layout, names, widest):
    """The cells of the compact window `w` scattered into the far buffer under the far strides of a row of `widest` bytes -- the arrays of
    a call share its one stride, so the narrower ones go as far as their rows take them -- 1 MiB apart.  Returns (the window's scalars
    with the far strides, {name: view}, the cells (T, n), {name: largest byte offset})."""
    ps, ts = far_strides(widest, layout)
    reach(widest, layout)
    _, _, total, at = geometry(N, T, layout, (ps, ts))
    t, b = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    compact = S.cell(t, b, w["ply_stride"], w["tile_stride"])
    views, tops = place(far, [(k, dt, tail, i << 20) for i, (k, dt, tail) in enumerate(WINDOW_NAMES) if k in names], at, total)
    for k in views:
        far.put(k, at, w[k][compact])
    return dict(n=N, plies=T, ply_stride=ps, tile_stride=ts), views, at, tops


@pytest.fixture(scope="module")
def windows(G):
    """130 boards x 3 plies of random rows, about 60 % of the cells of plies 1 and 2 valid, time- and tile-major, with a priority per
    cell (some zero)."""
    from tests.test_gpu_replay_prio import tile_major
    valid = np.random.default_rng(N).random((T, N)) < 0.6
    valid[0] = False
    w = S.synthetic_window(N, T, valid, seed=5)
    out = {}
    for layout in ("time", "tile"):
        x = dict(tile_major(w) if layout == "tile" else w)
        x["prio"] = np.random.default_rng(7).integers(0, 1000, len(x["z"])).astype(np.int32) * (np.random.default_rng(8).random(len(x["z"])) < 0.75)
        out[layout] = x
    return out, int(valid.sum())


@pytest.mark.parametrize("layout", ["time", "tile"])
def test_training_batch_reads_a_far_window(G, far, windows, layout):
    """All six arrays are required and share the stride: S is that of the observation rows (past 2^32); the visits rows end between 2^31
    and 2^32, the mask rows and the one-byte arrays below 2^31."""
    from tests.test_gpu_symmetry import device_batch
    w = windows[0][layout]
    names = ("obs", "mask", "visits", "z", "done", "mover")
    scalars, views, at, tops = far_window(far, w, layout, names, 117)
    exp = S.run_batch(nat.cpu_raw(), w, 256, 511, SEED, 1 << 33, 3)
    got = device_batch(nat.lib(), scalars, views, 256, 511, SEED, 1 << 33, 3)
    S.same_batch(got, exp)
    assert (exp["index"][:, 0] >= 0).sum() > 128
    cells = far.cells(at)
    t, b = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    compact = S.cell(t, b, w["ply_stride"], w["tile_stride"])
    assert all(np.array_equal(cells[k], w[k][compact]) for k in names), "the window was written"
    assert tops["obs"] >= 1 << 32 and 1 << 31 <= tops["visits"] < 1 << 32
    report("gbl_training_batch " + layout, tops)


@pytest.mark.parametrize("observations", [True, False], ids=["obs", "no_obs"])
@pytest.mark.parametrize("layout", ["time", "tile"])
def test_replay_appends_read_a_far_window(G, far, windows, layout, observations):
    """gbl_replay_append and gbl_replay_prio_append from a far window into a small compact ring, against the host flavour's appends of the
    compact window.  With observations S is that of the observation rows; without, that of the visits rows, which then pass 2^32."""
    from tests import replay_prio_restatement as P
    from tests import replay_restatement as R
    from tests.test_gpu_replay import DeviceRing, Guarded, device_append
    from tests.test_gpu_replay_prio import device_prio_append
    lib, cpu = nat.lib(), nat.cpu_raw()
    (w, K), tag = (windows[0][layout], windows[1]), (1 << 30) + 77
    names = ("obs",) * observations + ("mask", "visits", "z", "done", "mover", "prio")
    scalars, views, at, tops = far_window(far, w, layout, names, 117 if observations else 108)
    host, hprio = R.new_ring(512, observations, junk=1), np.zeros(512, np.int32)
    ring, dprio = DeviceRing(host), Guarded(hprio)
    R.run_append(cpu, host, w, tag)
    P.run_prio_append(cpu, host, hprio, w, w["prio"], 0)
    device_append(lib, ring, scalars, views, tag)
    device_prio_append(lib, ring, dprio, scalars, views, views["prio"], 0)
    torch.cuda.synchronize()
    ring.ws.read()  # (its guards)
    R.same_ring(ring.read(), host)
    assert np.array_equal(dprio.read(), hprio) and int(host["state"][0]) == K and (hprio > 0).sum() > K // 2
    cells = far.cells(at)
    t, b = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    compact = S.cell(t, b, w["ply_stride"], w["tile_stride"])
    assert all(np.array_equal(cells[k], w[k][compact]) for k in names), "the window was written"
    assert tops["obs" if observations else "visits"] >= 1 << 32
    report("gbl_replay_append + gbl_replay_prio_append %s %s" % (layout, "with observations" if observations else "without observations"), tops)
