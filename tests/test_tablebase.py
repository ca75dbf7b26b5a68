"""The exact tablebase, host flavour (no GPU): the gbl_cpu_tb_* entry points against the restatement of the header's paragraph
(tests/tablebase_restatement.py: the recursive V and the sweeps over whole universes), the index round trip, slices and sweeps in
place, the full inventory's 64-bit index arithmetic anchored to the engine (gbl_cpu_winner, gbl_cpu_solve), the probe on built and on
hand-filled tables, the colour symmetry the folded table rests on, Tablebase / TablebaseGobbletPolicy on the host flavour and the
recorded argument errors.

Inventories with three pieces a side ((1, 1, 1), (2, 1, 0), (0, 2, 1)) are decided after sweep 1: nobody can be forced.  The
deep sweeps are checked on (2, 2, 0), 2 024 929 positions and 40 sweeps."""
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import tablebase_harness as H
from tests import tablebase_restatement as R

DEEP = (2, 2, 0)


@pytest.fixture(scope="module", autouse=True)
def threads():
    nat.cpu_raw().gbl_cpu_set_threads(4)
    yield
    nat.cpu_raw().gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def deep():
    """(2, 2, 0) built by the host flavour in one call per sweep: (Host, table, counts)."""
    host = H.Host(DEEP)
    table, counts = host.build()
    assert len(counts) > 30 and counts[-1] == 0 and all(c > 0 for c in counts[:-1])
    table.setflags(write=False)
    return host, table, counts


# ---- layout, index and position ------------------------------------------------------------------------------------------------------
def test_layout():
    assert H.layout(H.FULL) == [H.FULL_POSITIONS, 1423, 1423, 1423, nat.TB_AUX_BYTES] and H.FULL_POSITIONS == 2881473967 < 1 << 32
    assert H.layout((1, 0, 2)) == [91 * 1423, 91, 1, 1423, nat.TB_AUX_BYTES]
    for inv in ((1, 1, 0), (2, 1, 0), (0, 0, 0)):
        assert H.layout(inv)[:4] == [R.Universe(inv).positions] + R.Universe(inv).L


def test_prepare_fills_the_tables_of_the_header():
    aux = H.Host((1, 1, 1)).aux
    U2, U1 = R.Universe((2, 0, 0)), R.Universe((1, 0, 0))
    rank2 = aux[0:2 * 19683].view(np.uint16)
    assert [int(rank2[t]) for t in U2.levels[0]] == list(range(1423)) and (rank2 == 0xFFFF).sum() == 19683 - 1423
    assert aux[39368:39368 + 2 * 1423].view(np.uint16).tolist() == U2.levels[0]
    assert aux[42216:42216 + 2 * 91].view(np.uint16).tolist() == U1.levels[0]
    assert aux[42400:42400 + 1024].view(np.uint16).tolist() == [sum(3 ** p for p in range(9) if m >> p & 1) for m in range(512)]
    rank1 = aux[43424:43424 + 19683]
    assert [int(rank1[t]) for t in U1.levels[0]] == list(range(91)) and (rank1 == 0xFF).sum() == 19683 - 91
    assert np.array_equal(aux, H.Host((2, 2, 2)).aux)  # (one aux for every inventory)


@pytest.mark.parametrize("inv", [(1, 1, 0), (2, 1, 0), (0, 2, 1), (0, 0, 0)])
def test_index_and_position_round_trip_over_whole_universes(inv):
    host, U = H.Host(inv), R.Universe(inv)
    idx = np.arange(host.positions)
    st = host.position(idx)
    assert np.array_equal(host.index(st, np.zeros(len(st), np.int8)), idx)
    assert np.array_equal(host.index(-st, np.ones(len(st), np.int8)), idx)      # player_2 to move: the colours swapped
    for i in np.random.default_rng(1).integers(0, host.positions, 200):
        assert np.array_equal(st[i], R.state_of(U.cells(int(i))))


def test_index_and_position_at_sampled_full_inventory_indices():
    host = H.Host(H.FULL)
    idx = np.array(H.FULL_SAMPLES + np.random.default_rng(2).integers(0, H.FULL_POSITIONS, 500).tolist(), np.int64)
    st = host.position(idx)
    assert np.array_equal(host.index(st, np.zeros(len(st), np.int8)), idx)
    assert np.array_equal(host.index(-st, np.ones(len(st), np.int8)), idx)
    U = R.Universe(H.FULL)
    for i, row in zip(idx[:40], st[:40]):
        assert np.array_equal(row, R.state_of(U.cells(int(i)))) and U.index(R.cells_of(row, 0)) == i
    assert (host.position(np.array(H.OUTSIDE, np.int64)) == nat.TB_TERMINAL).all()   # 2^32 +- 1 among them: no universe reaches 2^32
    # no states of the inventory: a third own piece on a level cannot be written as a contract state; a piece the inventory lacks can
    small = H.Host((1, 1, 0))
    rows = np.zeros((3, 27), np.int8)
    rows[0, 0], rows[1, 0], rows[2, 20] = 2, 1, 5   # piece 2 with c_0 = 1; fine; piece 5 with c_2 = 0
    assert small.index(rows, np.zeros(3, np.int8)).tolist() == [-1, small.index(rows[1:2], np.zeros(1, np.int8))[0], -1]


# ---- sweeps against the restatement ----------------------------------------------------------------------------------------------------
def test_every_sweep_of_a_small_universe_equals_the_recursive_value():
    """(1, 1, 0), 8 281 positions, the whole table after each of the sweeps 1 .. 5 against V(., k)."""
    host, U = H.Host((1, 1, 0)), R.Universe((1, 1, 0))
    assert host.positions == 8281
    V = R.V_factory(U)
    cells = [U.cells(i) for i in range(U.positions)]
    table = np.zeros(host.positions, np.int8)
    host.sweep(None, table, 0, host.positions, 0)
    terminal = np.array([R.winner(c) != 0 for c in cells])
    assert np.array_equal(table == nat.TB_TERMINAL, terminal) and (table[~terminal] == 0).all()
    for k in range(1, 6):
        host.sweep(table, table, 0, host.positions, k)
        exp = np.array([nat.TB_TERMINAL if t else V(c, k) for c, t in zip(cells, terminal)], np.int8)
        assert np.array_equal(table, exp), k


def test_the_first_sweeps_of_the_deep_universe_equal_the_recursive_value(deep):
    """(2, 2, 0): sampled positions after each of the sweeps 1 .. 3 against V(., k) -- here wins in 3 and losses in 2 exist."""
    host, _, _ = deep
    U = R.Universe(DEEP)
    V = R.V_factory(U)
    sample = np.random.default_rng(3).integers(0, host.positions, 150)
    table, _ = host.build(max_sweeps=0)
    seen = set()
    for k in range(1, 4):
        host.sweep(table, table, 0, host.positions, k)
        for i in sample:
            if table[i] != nat.TB_TERMINAL:
                assert table[i] == V(U.cells(int(i)), k), (k, i)
                seen.add(int(table[i]))
    assert {1, -2, 3, 0} <= seen


@pytest.mark.parametrize("inv", [(1, 1, 1), (2, 1, 0), (0, 2, 1)])
def test_the_fixed_point_equals_the_restatement_build(inv):
    host, U = H.Host(inv), R.Universe(inv)
    assert host.positions == U.positions and (inv != (1, 1, 1) or U.positions == 753571)
    table, counts = host.build()
    exp, exp_counts = R.build(U)
    assert counts == exp_counts and np.array_equal(table, exp)


def test_the_deep_fixed_point_is_consistent_with_its_own_children(deep):
    """(2, 2, 0), 40 sweeps: every sampled byte is the value the restatement's probe derives from the bytes of its successors, and the
    per-sweep counts are the table's own histogram."""
    host, table, counts = deep
    U = R.Universe(DEEP)
    assert counts[0] == int((table == nat.TB_TERMINAL).sum())
    for k in range(1, len(counts)):
        assert counts[k] == int((np.abs(table.astype(np.int16)) == k).sum())
    rng = np.random.default_rng(4)
    decided = np.nonzero((table != 0) & (table != nat.TB_TERMINAL))[0]
    late = np.nonzero(np.abs(table.astype(np.int16)) >= 20)[0]
    late = late[table[late] != nat.TB_TERMINAL]
    for i in np.concatenate([rng.choice(decided, 300), rng.choice(late, 100), rng.integers(0, host.positions, 200)]):
        if table[i] != nat.TB_TERMINAL:
            assert R.outcomes(U, table, R.state_of(U.cells(int(i))), 0)[1] == table[i], i


def test_slices_and_sweeps_in_place_give_the_bytes_of_whole_range_sweeps(deep):
    host, table, counts = deep
    sliced, sliced_counts = host.build(slices=H.ragged_slices(host.positions))
    assert sliced_counts == counts and np.array_equal(sliced, table)
    # not in place: sweep k of the whole range from the table after k - 1 into a buffer of its own
    cur, _ = host.build(max_sweeps=0)
    for k in range(1, 6):
        out = cur.copy()
        assert host.sweep(cur, out, 0, host.positions, k) == counts[k]
        assert np.array_equal(out != cur, np.abs(out.astype(np.int16)) == k)
        cur = out
    assert np.array_equal(np.where(np.abs(table.astype(np.int16)) <= 5, table, 0), np.where(cur == nat.TB_TERMINAL, 0, cur))
    # a slice into a buffer of its own, next to the universe it reads
    first, count = 1000, 777
    part = cur[first:first + count].copy()
    host.sweep(cur, part, first, count, 6)
    assert np.array_equal(np.abs(part.astype(np.int16)) == 6, np.abs(table[first:first + count].astype(np.int16)) == 6)


def test_full_inventory_slices_agree_with_the_engine():
    """(2, 2, 2), sweep 0 and sweep 1 of slices of 4 096 positions at 0, across 2^31 and at the end, table = NULL: the bytes against
    gbl_cpu_winner and gbl_cpu_solve(depth = 1) on the positions gbl_cpu_tb_position returns."""
    host, L = H.Host(H.FULL), nat.cpu_raw()
    for first in H.FULL_SLICES:
        idx = np.arange(first, first + H.SLICE, dtype=np.int64)
        st, tm = host.position(idx), np.zeros(H.SLICE, np.int8)
        win, val = np.zeros(H.SLICE, np.int8), np.zeros(H.SLICE, np.int8)
        assert L.gbl_cpu_winner(st.ctypes.data, win.ctypes.data, H.SLICE, None) == 0
        assert L.gbl_cpu_solve(st.ctypes.data, tm.ctypes.data, None, 1, None, val.ctypes.data, None, H.SLICE, None) == 0
        out = np.full(H.SLICE, 0x5A, np.int8)
        assert host.sweep(None, out, first, H.SLICE, 0) == int((win != 0).sum())
        assert np.array_equal(out, np.where(win != 0, nat.TB_TERMINAL, 0))
        wrote = host.sweep(None, out, first, H.SLICE, 1)
        exp = np.where(win != 0, nat.TB_TERMINAL, val)
        assert np.array_equal(out, exp) and wrote == int(((win == 0) & (val != 0)).sum())
        assert first != 0 or {1, 0, nat.TB_TERMINAL} <= set(out.tolist())


# ---- the probe -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv", [(1, 1, 1), (2, 1, 0), DEEP])
def test_probe_equals_the_restatement(inv, deep):
    host = deep[0] if inv == DEEP else H.Host(inv)
    table = deep[1] if inv == DEEP else host.build()[0]
    U = R.Universe(inv)
    st, tm = H.sample_boards(host, 120, 5)
    mask = (np.random.default_rng(6).random((len(st), 54)) < 0.7).astype(np.int8)
    for m in (None, mask):
        got, exp = host.probe(table, st, tm, m), H.expected_probe(U, table, st, tm, m)
        for k in got:
            assert np.array_equal(got[k], exp[k]), (k, np.argwhere(got[k] != exp[k])[:5])
    if inv == DEEP:
        assert len(set(got["value"].tolist())) > 5


def test_probe_on_a_table_of_chosen_bytes():
    """The c(a) formula, the rank order, ties, the mask, GBL_SOLVE_NONE, roots without a candidate, player_2 through the fold and NULL
    outputs, on a (1, 1, 1) table the test fills itself: every byte in -126 .. 126 and GBL_TB_TERMINAL occurs."""
    host, U = H.Host((1, 1, 1)), R.Universe((1, 1, 1))
    rng = np.random.default_rng(7)
    table = rng.integers(-126, 127, host.positions).astype(np.int8)
    table[rng.random(host.positions) < 0.2] = 0
    table[rng.random(host.positions) < 0.05] = nat.TB_TERMINAL
    st, tm = H.sample_boards(host, 150, 8)
    mask = (rng.random((len(st), 54)) < 0.5).astype(np.int8)
    mask[3] = 0                       # a root without a candidate
    st[5], st[5][0] = 0, 2            # piece 2 with c_0 = 1: no state of the inventory
    exp = H.expected_probe(U, table, st, tm, mask)
    got = host.probe(table, st, tm, mask)
    for k in got:
        assert np.array_equal(got[k], exp[k]), (k, np.argwhere(got[k] != exp[k])[:5])
    for b in (3, 5):
        assert (got["outcome"][b] == nat.SOLVE_NONE).all() and got["value"][b] == 0 and got["action"][b] == -1
    assert {-127, 127, 0} <= set(got["outcome"].reshape(-1).tolist()) and (got["outcome"][:, 18:] != nat.SOLVE_NONE).any()
    assert (got["outcome"].reshape(len(st), 6, 9)[:, 1::2] == nat.SOLVE_NONE).all()   # pieces 2, 4, 6 do not exist
    # constant tables: every quiet action ties, the lowest index decides; a win at once outranks everything
    for byte, c in ((0, 0), (9, -10), (-9, 10), (nat.TB_TERMINAL, 0)):
        flat = host.probe(np.full(host.positions, byte, np.int8), st, tm, mask)
        e = H.expected_probe(U, np.full(host.positions, byte, np.int8), st, tm, mask)
        assert all(np.array_equal(flat[k], e[k]) for k in flat)
        quiet = (flat["outcome"] != nat.SOLVE_NONE) & (np.abs(flat["outcome"]) != 1)
        assert (flat["outcome"][quiet] == c).all()
    for keep in (("value",), ("action",), ("outcome",), ()):
        part = host.probe(table, st, tm, mask, keep)
        assert set(part) == set(keep) and all(np.array_equal(part[k], exp[k]) for k in keep)


def test_the_solver_commutes_with_the_colour_swap():
    """The fold rests on this: gbl_cpu_solve gives the same V and the same outcome rows on a board and on its colour-swapped twin with
    the other side to move."""
    host, L = H.Host(H.FULL), nat.cpu_raw()
    st, tm = H.sample_boards(host, 256, 9, renumber=False)
    st, tm = np.where(tm[:, None] == 1, -st, st).astype(np.int8), np.zeros(len(st), np.int8)   # all from player_1's side
    from tests.search_harness import midgame_boards, run
    real, real_tm = midgame_boards(64, "cpu")
    st, tm = np.concatenate([st, real]), np.concatenate([tm, real_tm])
    for depth in (1, 3):
        a = run("solve", "cpu", st, tm, None, (depth,))
        b = run("solve", "cpu", (-st).astype(np.int8), (1 - tm).astype(np.int8), None, (depth,))
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert len(set(a["value"].tolist())) >= 3


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_tablebase_class_build_probe_save_and_load(tmp_path):
    tb = G.Tablebase((2, 1, 0), "cpu")
    assert tb.positions == 129493 and not tb.complete and tb.sweeps == 0
    assert tb.build(max_sweeps=1) == [9636] and tb.sweeps == 1 and not tb.complete
    counts = tb.build(slice_positions=50000)
    exp, exp_counts = R.build(R.Universe((2, 1, 0)))
    assert counts == exp_counts == tb.decided and tb.complete and tb.sweeps == len(counts)
    assert np.array_equal(tb.table.numpy(), exp) and tb.build() == counts   # (a complete table sweeps no more)
    host = H.Host((2, 1, 0))
    st, tm = H.sample_boards(host, 64, 10)
    got = tb.probe(st, tm)
    raw = host.probe(exp, st, tm)
    assert all(np.array_equal(got[k].numpy(), raw[k]) for k in raw)
    idx = tb.index(st, tm)
    assert (idx >= 0).all() and np.array_equal(tb.value(idx).numpy(), exp[idx.numpy()])
    assert np.array_equal(tb.index(tb.position(idx), np.zeros(64, np.int8)).numpy(), idx.numpy())
    path = str(tmp_path / "tb.bin")
    tb.save(path)
    assert os.path.getsize(path) == G.tablebase.HEADER_BYTES + tb.positions
    again = G.Tablebase.load(path, "cpu")
    assert (again.inventory, again.sweeps, again.complete, again.decided) == (tb.inventory, tb.sweeps, True, tb.decided)
    assert torch.equal(again.table, tb.table) and all(torch.equal(again.probe(st, tm)[k], got[k]) for k in got)
    with open(path, "r+b") as f:
        f.truncate(G.tablebase.HEADER_BYTES + 1000)
    with pytest.raises(ValueError):
        G.Tablebase.load(path, "cpu")
    with pytest.raises(ValueError):
        G.Tablebase((3, 1, 0), "cpu")
    # the header holds the longest list a build can leave: 127 counts of ten digits
    small = G.Tablebase((1, 0, 0), "cpu")
    small.sweeps, small.decided = 127, [2881473967] * 127
    small.save(path)
    assert G.Tablebase.load(path, "cpu").decided == small.decided


def test_build_stops_before_sweep_127():
    tb = G.Tablebase((1, 0, 0), "cpu")
    tb.build(max_sweeps=1)
    tb.sweeps = nat.TB_MAX_SWEEP        # as if 126 sweeps had each decided something
    tb.build(max_sweeps=1)
    assert tb.sweeps == 127 and tb.complete   # (sweep 126 itself is fine; here it decided nothing)
    tb.complete = False
    with pytest.raises(nat.GobbletHipError, match="127"):
        tb.build(max_sweeps=1)
    assert tb.sweeps == 127 and (tb.table.abs() <= 126).all()


def test_policy_with_and_without_a_fallback(deep):
    host, table, counts = deep
    tb = G.Tablebase(DEEP, "cpu")
    tb.table.copy_(torch.from_numpy(table.copy()))
    tb.sweeps, tb.complete, tb.decided = len(counts), True, counts
    st, tm = H.sample_boards(host, 200, 11)
    pol = G.TablebaseGobbletPolicy(tb)
    act = pol.compute_actions_from_state(st, tm)
    raw = host.probe(table, st, tm)
    assert np.array_equal(act.numpy(), raw["action"]) and np.array_equal(pol.last_outcomes.numpy(), raw["outcome"])
    assert np.array_equal(pol.last_value.numpy(), raw["value"]) and np.array_equal(pol.outcomes(st, tm).numpy(), raw["outcome"])
    drawn = raw["value"] == 0
    assert drawn.any() and (~drawn).any()

    class Highest:   # a fallback that takes the highest action its mask allows
        device = torch.device("cpu")

        def compute_actions_from_state(self, state, to_move, mask):
            self.mask = mask
            return (53 - mask.flip(1).to(torch.int32).argmax(1)).to(torch.int32)

    fb = Highest()
    both = G.TablebaseGobbletPolicy(tb, fallback=fb).compute_actions_from_state(st, tm).numpy()
    assert np.array_equal(both[~drawn], raw["action"][~drawn])
    zero = raw["outcome"] == 0
    assert np.array_equal(fb.mask.numpy().astype(bool), zero[drawn]) and (both[drawn] == 53 - zero[drawn][:, ::-1].argmax(1)).all()
    assert (both[drawn] != raw["action"][drawn]).any()
    # the environment's own boards
    env = G.BatchedGobblet(8, "cpu")
    out = env.tablebase(tb)
    assert all(torch.equal(out[k], tb.probe(np.zeros((8, 27), np.int8), np.zeros(8, np.int8))[k]) for k in out)
    assert (out["outcome"][:, 36:] == nat.SOLVE_NONE).all() and (out["outcome"][:, :36] != nat.SOLVE_NONE).all()


# ---- argument errors --------------------------------------------------------------------------------------------------------------------
def test_tablebase_argument_errors_replay_the_recorded_table(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "tablebase_arg_errors.json")))
    assert len(table) > 40 and {c["fn"] for c in table} == {"tb_layout", "tb_prepare", "tb_sweep", "tb_index", "tb_position", "tb_probe"}
    H.replay_tb_arg_errors(table)
