"""Board symmetries and symmetry-augmented training batches, host flavour (no GPU): gbl_cpu_symmetry_apply and gbl_cpu_training_batch
against the numpy restatement of the header's text (tests/symmetry_restatement.py), the group laws, and -- against the ORACLE -- that
the rules commute with the group: legal mask, observation and a step everywhere, check_for_winner on every board that does not hold a
line of each colour, the solver under the piece swaps."""
import json
import os

import numpy as np
import pytest

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from gobblet_rl_amd import symmetry as S
from tests import solver_restatement as SR
from tests.search_harness import replay_arg_errors, run
from tests import symmetry_restatement as R

LINES = ((0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6))
SWAPS = (0b000000, 0b101011, 0b010110, 0b111111)  # four of the 64 swap patterns: none, two mixed ones, all six pairs


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


def random_rows(n, seed):
    """One row of every type per board: contract-shaped states and arbitrary bytes elsewhere (the transform only moves them)."""
    rng = np.random.default_rng(seed)
    level = np.repeat(np.arange(3), 9)
    state = (rng.integers(0, 3, (n, 27)) * rng.choice([-1, 1], (n, 27)))
    state = np.where(state != 0, np.sign(state) * (2 * level + np.abs(state)), 0).astype(np.int8)
    actions = rng.integers(0, 54, n).astype(np.int32)
    actions[::7], actions[3::11] = -1, 54
    return dict(state=state, obs=rng.integers(-128, 128, (n, 117)).astype(np.int8), mask=rng.integers(-128, 128, (n, 54)).astype(np.int8),
                visits=rng.integers(-32768, 32768, (n, 54)).astype(np.int16), priors=rng.integers(0, 256, (n, 54)).astype(np.uint8),
                actions=actions)


def golden_rows(golden_dir, n=512):
    """n boards of the golden set (repeated to n) with every row type the library derives from them."""
    sq = np.load(os.path.join(golden_dir, "board_functions.npz"))["squares"]
    state = np.ascontiguousarray(sq[np.arange(n) % len(sq)])
    agent = (np.arange(n) // len(sq) + np.arange(n)) % 2
    agent = agent.astype(np.int8)
    rng = np.random.default_rng(1)
    mask = oracle.batch_legal_mask(state, agent)
    return agent, dict(state=state, obs=oracle.batch_observe(state, agent).reshape(n, 117), mask=mask,
                       visits=(mask * rng.integers(1, 1024, (n, 54))).astype(np.int16), priors=(mask * rng.integers(1, 256, (n, 54))).astype(np.uint8),
                       actions=rng.integers(0, 54, n).astype(np.int32))


# ---- the group ---------------------------------------------------------------------------------------------------------------------
def test_the_512_codes_are_distinct_and_the_python_maps_restate_the_header():
    seen = {(tuple(R.sigma(s)), tuple(R.tau(s, 0)), tuple(R.tau(s, 1))) for s in range(512)}
    assert len(seen) == 512 == S.N_SYMMETRIES == G.N_SYMMETRIES
    act_to = R.tables()[2]
    for s in range(512):
        assert S.position_map(s) == R.sigma(s)
        for m in (0, 1):
            assert S.action_map(s, m) == act_to[s, m].tolist() and sorted(S.action_map(s, m)) == list(range(54))
    assert S.position_map(1) == [2, 5, 8, 1, 4, 7, 0, 3, 6] and S.position_map(4) == [2, 1, 0, 5, 4, 3, 8, 7, 6]  # a quarter turn; the mirror
    assert S.action_map(8, 0)[:18] == list(range(9, 18)) + list(range(9)) and S.action_map(8, 1) == list(range(54))
    with pytest.raises(ValueError):
        S.position_map(512)


def test_group_laws_on_every_row_type(cpu, golden_dir):
    """apply(compose(g, h)) == apply(g) o apply(h) and apply(inverse(g)) o apply(g) == id, every code used as g and as h."""
    agent, rows = golden_rows(golden_dir)
    n = len(agent)
    rng = np.random.default_rng(2)
    g, h = rng.permutation(512).astype(np.int16), rng.permutation(512).astype(np.int16)
    assert len(set(g.tolist())) == 512 == len(set(h.tolist()))
    gh = np.array([S.compose(int(a), int(b)) for a, b in zip(g, h)], np.int16)
    ginv = np.array([S.inverse(int(a)) for a in g], np.int16)
    assert all(S.compose(int(a), int(b)) == 0 == S.compose(int(b), int(a)) for a, b in zip(g, ginv))
    after_h = R.run_apply(cpu, h, agent, **rows)
    after_gh = R.run_apply(cpu, g, agent, **after_h)
    direct = R.run_apply(cpu, gh, agent, **rows)
    back = R.run_apply(cpu, ginv, agent, **R.run_apply(cpu, g, agent, **rows))
    changed = 0
    for k in R.ROWS:
        assert np.array_equal(after_gh[k], direct[k]), k
        assert np.array_equal(back[k], rows[k]), k
        changed += int((direct[k] != rows[k]).any())
    assert changed == len(R.ROWS)  # (nothing above is the identity's doing)


# ---- host flavour == restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_apply_host_flavour_equals_restatement(cpu, n):
    rows = random_rows(n, seed=n)
    rng = np.random.default_rng(n + 1)
    agent = rng.integers(0, 2, n).astype(np.int8) * rng.choice(np.array([1, -1, 2, 127], np.int8), n)  # (non-zero = player_2)
    sym = rng.integers(0, 512, n).astype(np.int16)
    same = lambda got, exp: [np.testing.assert_array_equal(got[k], exp[k], err_msg=k) for k in exp]  # noqa: E731
    same(R.run_apply(cpu, sym, agent, **rows), R.apply(sym, agent, **rows))
    high = (sym | np.int16(-512)).astype(np.int16)  # only the low 9 bits are read
    same(R.run_apply(cpu, high, agent, **rows), R.apply(sym, agent, **rows))
    for s in (0, 5, 0b101010111, 511):  # the scalar for every board
        same(R.run_apply(cpu, s, agent, **rows), R.apply(np.full(n, s), agent, **rows))
    same(R.run_apply(cpu, sym, None, state=rows["state"]), R.apply(sym, None, state=rows["state"]))  # state alone needs no agent
    sub = {k: rows[k] for k in ("obs", "actions")}
    same(R.run_apply(cpu, sym, agent, **sub), R.apply(sym, agent, **sub))
    ident = R.run_apply(cpu, 0, agent, **rows)
    assert all(np.array_equal(ident[k], rows[k]) for k in rows)


def test_python_apply_on_the_host_flavour():
    import torch
    n = 70
    rows = random_rows(n, seed=9)
    agent = (np.arange(n) % 2).astype(np.int8)
    sym = np.random.default_rng(10).integers(0, 512, n)
    t = {k: torch.from_numpy(v) for k, v in rows.items()}
    got = S.apply(torch.from_numpy(sym), torch.from_numpy(agent), state=t["state"], observation=t["obs"].reshape(n, 3, 3, 13),
                  action_mask=t["mask"], visits=t["visits"], priors=t["priors"], actions=t["actions"])
    exp = R.apply(sym, agent, **rows)
    names = {"state": "state", "observation": "obs", "action_mask": "mask", "visits": "visits", "priors": "priors", "actions": "actions"}
    assert set(got) == set(names) and got["observation"].shape == (n, 3, 3, 13)
    for k, r in names.items():
        assert np.array_equal(got[k].numpy().reshape(exp[r].shape), exp[r]), k
    one = S.apply(77, state=t["state"])
    assert set(one) == {"state"} and np.array_equal(one["state"].numpy(), R.apply(np.full(n, 77), state=rows["state"])["state"])
    with pytest.raises(ValueError):
        S.apply(3, action_mask=t["mask"])       # needs agent
    with pytest.raises(ValueError):
        S.apply(512, state=t["state"])


# ---- the rules commute, against the oracle -----------------------------------------------------------------------------------------
def rule_boards(golden_dir):
    """(state, to_move): the golden boards, movers alternating, and a seeded masked-random mix of 20 480 boards at 2 .. 24 plies.  (The
    golden set carries 17 hand-built boards with a line of each colour among its 408, 4 %: the mix is sized so that the excluded share of
    the whole set stays inside the 0.2 % the winner comparison allows.)"""
    sq = np.load(os.path.join(golden_dir, "board_functions.npz"))["squares"]
    st, tm = [sq], [(np.arange(len(sq)) % 2).astype(np.int8)]
    for t in (2, 4, 6, 8, 10, 12, 14, 16, 20, 24):
        s, m, d = oracle.batch_reset(2048)
        oracle.batch_rollout(s, m, d, 100 + t, 0, 0, t, want_obs=False, want_mask=False)
        st.append(s)
        tm.append(m)
    return np.ascontiguousarray(np.concatenate(st)), np.ascontiguousarray(np.concatenate(tm))


def holds_a_line_of_each_colour(state):
    flat = oracle.batch_flatboard(state)
    pos = np.zeros(len(state), bool)
    neg = np.zeros(len(state), bool)
    for a, b, c in LINES:
        pos |= (flat[:, a] > 0) & (flat[:, b] > 0) & (flat[:, c] > 0)
        neg |= (flat[:, a] < 0) & (flat[:, b] < 0) & (flat[:, c] < 0)
    return pos & neg


def test_rules_commute_with_the_group(cpu, golden_dir):
    st, tm = rule_boards(golden_dir)
    n = len(st)
    assert n >= 8192 + 408 and set(tm[408:].tolist()) == {0, 1}
    mask = oracle.batch_legal_mask(st, tm)
    obs = oracle.batch_observe(st, tm).reshape(n, 117)
    # a seeded legal action per board (-1 where the mover has none), and the position after it
    rng = np.random.default_rng(7)
    pick = (rng.random(n) * mask.sum(1)).astype(np.int64)
    act = np.where(mask.any(1), np.argmax(np.cumsum(mask != 0, 1) > pick[:, None], 1), -1).astype(np.int32)
    assert all(mask[b, act[b]] for b in range(0, n, 97) if act[b] >= 0)
    nxt, nxt_tm = st.copy(), tm.copy()
    oracle.batch_step(nxt, nxt_tm, np.zeros(n, np.int8), act, want_obs=False, want_mask=False)
    win, win_nxt = oracle.batch_winner(st), oracle.batch_winner(nxt)
    both = np.concatenate([st, nxt])
    dual = holds_a_line_of_each_colour(both)
    assert dual.mean() <= 0.002, dual.mean()   # condition of the test, not a measurement (measured: 0.04 % of masked-random play)
    assert (win != 0).sum() + (win_nxt != 0).sum() > 100   # (decided boards are in the set)
    for code in [sq | (sw << 3) for sq in range(8) for sw in SWAPS]:
        img = R.run_apply(cpu, code, tm, state=st, obs=obs, mask=mask, actions=act)
        g_st = img["state"]
        assert np.array_equal(oracle.batch_legal_mask(g_st, tm), img["mask"]), code
        assert np.array_equal(oracle.batch_observe(g_st, tm).reshape(n, 117), img["obs"]), code
        g_nxt, g_tm = g_st.copy(), tm.copy()
        oracle.batch_step(g_nxt, g_tm, np.zeros(n, np.int8), img["actions"], want_obs=False, want_mask=False)
        assert np.array_equal(g_nxt, R.run_apply(cpu, code, None, state=nxt)["state"]) and np.array_equal(g_tm, nxt_tm), code
        g_win = oracle.batch_winner(np.concatenate([g_st, g_nxt]))
        assert np.array_equal(g_win[~dual], np.concatenate([win, win_nxt])[~dual]), code
        assert np.array_equal(holds_a_line_of_each_colour(np.concatenate([g_st, g_nxt])), dual), code


def test_solver_commutes_with_the_piece_swaps(cpu):
    """sigma = identity: exact by the rules, so gbl_cpu_solve(depth 3) of the image is the image of its outcomes -- on 256 boards, the
    zugzwang boards among them."""
    parts = [SR.rollout_positions(10), SR.zugzwang(), SR.hand_built()]
    st, tm = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert len(st) == 256
    out, val, _ = run("solve", "cpu", st, tm, None, (3,)).values()
    codes = ((np.arange(256) * 29 + 1) % 64).astype(np.int16) << 3   # every swap pattern, four boards each
    assert len(set(codes.tolist())) == 64 and (codes & 7 == 0).all()
    g_st = R.run_apply(cpu, codes, None, state=st)["state"]
    g_out, g_val, g_act = run("solve", "cpu", g_st, tm, None, (3,)).values()
    assert np.array_equal(g_out, R.run_apply(cpu, codes, tm, mask=out)["mask"]) and np.array_equal(g_val, val)
    assert (g_out != out).any() and (out[256 - 4] == 2).any()   # (ZUG_NODE's win in two is there)
    has = g_act >= 0
    assert [SR.rank(int(c)) for c in g_out[has, g_act[has]]] == [SR.rank(int(v)) for v in val[has]]


# ---- training batches --------------------------------------------------------------------------------------------------------------
SEED, BASE = 0x1234567890ABCDEF, (1 << 40) + 5


@pytest.mark.parametrize("boards,plies,layout", R.WINDOWS)
def test_training_batch_host_flavour_equals_restatement(cpu, boards, plies, layout):
    w = R.host_window(boards, plies, layout)
    ok = R.valid_cells(w)
    assert 0.3 < ok[1:].mean() < 0.95, ok[1:].mean()
    assert (w["tile_stride"] == 64) == (layout == "time")
    failed_total = 0
    for call in (0, (1 << 26) - 1):
        for sym_mask in (0, 7, 511):
            exp, failed = R.training_batch(w, 1000, sym_mask, SEED, BASE, call)
            failed_total += failed
            for batch in (1, 63, 65, 1000):
                got = R.run_batch(cpu, w, batch, sym_mask, SEED, BASE, call)
                R.same_batch(got, exp, batch)   # (a batch is the beginning of every longer one: the draw does not depend on `batch`)
            t, b = exp["index"][exp["index"][:, 0] >= 0].T
            assert ok[t, b].all()
            if sym_mask == 0:
                at, prev = R.cell(t, b, w["ply_stride"], w["tile_stride"]), R.cell(t - 1, b, w["ply_stride"], w["tile_stride"])
                keep = exp["index"][:, 0] >= 0
                assert np.array_equal(exp["obs"][keep], w["obs"][prev]) and np.array_equal(exp["visits"][keep], w["visits"][at])
                assert np.array_equal(exp["mask"][keep], w["mask"][prev]) and not exp["sym"].any()
            else:
                assert exp["sym"].max() <= sym_mask and len(set(exp["sym"].tolist())) > min(sym_mask, 200) * 0.9
    assert failed_total < 0.01 * 6 * 1000   # condition (the valid share of such windows is 0.56-0.76: about 1e-6 per sample)
    assert not np.array_equal(R.run_batch(cpu, w, 63, 511, SEED, BASE, 0)["index"], R.run_batch(cpu, w, 63, 511, SEED, BASE, 1)["index"])
    assert np.array_equal(R.run_batch(cpu, w, 64, 511, SEED, BASE + 1, 0)["index"][:63], R.run_batch(cpu, w, 64, 511, SEED, BASE, 0)["index"][1:])


def test_training_batch_returns_the_plies_the_trainer_keeps():
    """Through BatchedGobblet.training_batch: every (t, b) is in the keep set of examples/example_train_evaluator.py's targets_of, and the
    rows are the images of the window's rows."""
    import torch
    boards, plies = 200, 12
    env = G.BatchedGobblet(boards, "cpu", auto_reset=True, seed=3, track_turn=True)
    traj = env.collect(plies, policies=("tree", "tree"), search=R.SEARCH)
    with pytest.raises(ValueError, match="outcome_targets"):
        env.training_batch(traj, 8)
    env.outcome_targets(traj)
    z, visits = traj["z"][1:], traj["visits"][1:].float()
    keep = (z != nat.Z_OPEN) & (traj["done"][:-1] == 0) & (visits.sum(-1) > 0)   # targets_of's
    w = R.window_of(traj, boards)
    assert np.array_equal(R.valid_cells(w)[1:], keep.numpy())
    for symmetries, sym_mask in (("all", 511), ("square", 7), (None, 0)):
        out = env.training_batch(traj, 500, symmetries=symmetries, call=4)
        exp, _ = R.training_batch(w, 500, sym_mask, env.seed, 0, 4)
        assert out["observation"].shape == (500, 117) and out["index"].dtype == torch.int32
        for k, r in (("observation", "obs"), ("action_mask", "mask"), ("visits", "visits"), ("z", "z"), ("index", "index"), ("sym", "sym")):
            assert np.array_equal(out[k].numpy(), exp[r]), (symmetries, k)
        t, b = out["index"].long().T
        assert bool(keep[t - 1, b].all())
    again = env.training_batch(traj, 500, symmetries=None, call=4, out=out)
    assert again is out
    for bad in ({k: v for k, v in out.items() if k != "observation"}, {**out, "visits": out["visits"][:499]},
                {**out, "z": out["z"].to(torch.int16)}):
        with pytest.raises(ValueError, match="out"):
            env.training_batch(traj, 500, out=bad)
    with pytest.raises(ValueError, match="out"):
        env.training_batch(traj, 499, out=out)
    with pytest.raises(ValueError):
        env.training_batch(traj, 8, symmetries="diagonal")


def test_the_training_example_fits_on_augmented_batches():
    """examples/example_train_evaluator.py --augment: a few Adam steps on batches drawn by training_batch, on the host flavour."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_train_evaluator", os.path.join(root, "examples", "example_train_evaluator.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    for augment in ("square", "all"):
        ev, kept, loss = ex.train_evaluator("cpu", boards=64, plies=12, steps=3, hidden=64, collect_iterations=8, augment=augment)
        assert isinstance(ev, G.GobbletEvaluator) and kept > 100 and np.isfinite(loss) and loss > 0


def test_training_batch_edge_windows(cpu):
    # every z open: every sample fails
    w = R.synthetic_window(70, 5, np.zeros((5, 70), bool))
    got = R.run_batch(cpu, w, 65, 511, 1, 0, 0)
    assert not got["obs"].any() and not got["mask"].any() and not got["visits"].any() and not got["sym"].any()
    assert (got["index"] == -1).all() and (got["z"] == R.Z_OPEN).all()
    R.same_batch(got, R.training_batch(w, 65, 511, 1, 0, 0)[0])
    # plies = 2: t is always 1
    valid = np.zeros((2, 130), bool)
    valid[1, ::2] = True
    w = R.synthetic_window(130, 2, valid)
    got = R.run_batch(cpu, w, 200, 511, 2, 0, 0)
    exp, failed = R.training_batch(w, 200, 511, 2, 0, 0)
    R.same_batch(got, exp)
    assert failed < 3 and set(got["index"][:, 0].tolist()) <= {1, -1} and (got["index"][got["index"][:, 0] > 0, 1] % 2 == 0).all()
    # the only valid cells lie in the one board of a ragged last tile
    valid = np.zeros((6, 65), bool)
    valid[1:, 64] = True
    w = R.synthetic_window(65, 6, valid)
    got = R.run_batch(cpu, w, 300, 7, 3, 0, 0)
    exp, failed = R.training_batch(w, 300, 7, 3, 0, 0)
    R.same_batch(got, exp)
    hit = got["index"][:, 0] >= 0
    assert 10 < hit.sum() < 150 and failed == 300 - hit.sum() and (got["index"][hit, 1] == 64).all()   # (16 attempts at 1 / 65 each)
    # a done flag in slot t - 1 and an unvisited ply take a cell out
    valid = np.ones((3, 64), bool)
    valid[0] = False
    w = R.synthetic_window(64, 3, valid)
    w["done"][R.cell(0, 5, 64, 64)] = 1
    w["visits"][R.cell(2, 9, 64, 64)] = 0
    w["visits"][R.cell(1, 9, 64, 64)] = np.where(np.arange(54) % 2, -3, 3)   # (sums to zero: not "more than 0")
    ok = R.valid_cells(w)
    assert not ok[1, 5] and ok[2, 5] and not ok[2, 9] and not ok[1, 9] and ok.sum() == 128 - 3
    got = R.run_batch(cpu, w, 2000, 511, 4, 0, 0)
    R.same_batch(got, R.training_batch(w, 2000, 511, 4, 0, 0)[0])
    assert ok[got["index"][:, 0], got["index"][:, 1]].all()


def test_batch_argument_errors_replay_the_recorded_table(golden_dir):
    """tests/golden/batch_arg_errors.json: bad calls of gbl_symmetry_apply and gbl_training_batch with the return code and the
    gbl_last_error text of either flavour.  Every call returns before any device work (the pointers are numbers, never read); a case
    whose "host" is null is an alignment rule, which only the device flavour has."""
    table = json.load(open(os.path.join(golden_dir, "batch_arg_errors.json")))
    assert len(table) > 40 and {c["fn"] for c in table} == {"symmetry_apply", "training_batch"}
    replay_arg_errors(table)
