"""gbl_cpu_collect_search_tb on the host flavour (no GPU): against the restatement of the header text
(tests/selfplay_tb_restatement.py) on a complete table and on pseudo-random bytes, its equality with gbl_cpu_collect_search_noise, the
properties perfect play must have, the cross-pin with gbl_cpu_tb_targets, the recorded argument errors of both flavours, the Python
surface on device="cpu" and Tablebase.judge."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as ER
from tests import selfplay_tb_harness as H
from tests import selfplay_tb_restatement as R
from tests import tablebase_harness as TH
from tests import tb_targets_harness as TT
from tests import tb_targets_restatement as TR
from tests.search_harness import replay_arg_errors
from tests.selfplay_harness import SOLVE_NAMES, same
from tests.test_selfplay_solve import collect_solve, smoke_net

DEEP, WIDE = (2, 2, 0), (1, 1, 2)
SEED, ENV_BASE = 0x0123456789ABCDEF, (1 << 40) + 5
TABLE_HOWS = (nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED)


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def deep(cpu):
    """The complete (2, 2, 0) table, built once: (host, H.Table)."""
    host = TH.Host(DEEP)
    table, counts = host.build()
    assert counts[-1] == 0
    return host, H.Table(DEEP, host.aux, table)


@pytest.fixture(scope="module")
def wide(cpu):
    """Pseudo-random bytes over (1, 1, 2) holding every byte value (+-126, +-127 and GBL_TB_TERMINAL among the children)."""
    host = TH.Host(WIDE)
    return host, H.Table(WIDE, host.aux, TT.random_table(host.positions, 3))


def probe_of(host, tb):
    return lambda st, tm: host.probe(tb.table, st, tm)


# ---- against the restatement ----------------------------------------------------------------------------------------------------------
POLICIES = [(("tb", "tb"), (0, 0), (0, 0), (0, 0), True), (("tb", "random"), (0, 0), (0, 0), (0, 0), True),
            (("random", "tb"), (0, 0), (0, 0), (0, 0), False), (("eval", "tb"), (6, 0), (2, 0), (64, 0), True),
            (("eval", "eval"), (5, 4), (0, 2), (0, 0), True)]  # policies, iterations, guard depths, noise weights, judge
# layout, illegal mode, sample_plies, tb_mode, tb_count, ply_dev: every value of each on two rows
WINDOWS = [("time", nat.ILLEGAL_NOOP, 0, 0, 1, None), ("tile", nat.ILLEGAL_TERMINATE, 2, 1, 600, 3),
           ("time", nat.ILLEGAL_TERMINATE, 2, 0, 600, None), ("tile", nat.ILLEGAL_NOOP, 0, 1, 1, 5)]
T, X, PLY0 = 5, 24, 9


@pytest.mark.parametrize("which", ["deep", "wide"])
@pytest.mark.parametrize("case", POLICIES, ids=lambda c: "-".join(c[0]) + ("-judge" if c[4] else ""))
def test_host_flavour_equals_restatement(request, cpu, which, case):
    host, tb = request.getfixturevalue(which)
    pols, its, deps, noise, judge = case
    st, tm, turn = H.start_boards(host, 6, 4, 2, seed=17)
    nets = tuple(smoke_net() if p == "eval" and m == 0 else ER.random_net(128, 77) if p == "eval" else None for m, p in enumerate(pols))
    keep = None if judge else [k for k, _, _ in SOLVE_NAMES]
    hows = set()
    for layout, illegal_mode, sample_plies, mode, count, ply_dev in WINDOWS:
        exp = R.restate_collect_tb(probe_of(host, tb), st, tm, turn, T, pols, nets, its, deps, noise, X, sample_plies, illegal_mode, SEED,
                                   ENV_BASE, PLY0, mode, count, judge)
        if not judge:
            exp = ({k: v for k, v in exp[0].items() if k in keep},) + exp[1:]
        got = H.host_collect_tb(tb, st, tm, turn, T, pols, nets, its, deps, noise, X, sample_plies, illegal_mode, layout, SEED, ENV_BASE,
                                PLY0 - (ply_dev or 0), ply_dev, mode, count, keep)
        same(got, exp)
        hows |= set(got[0]["how"].ravel().tolist())
        tr = got[0]
        labelled = np.isin(tr["how"], TABLE_HOWS)
        assert not tr["priors"][labelled].any() and not tr["nodes"][labelled].any() and not tr["root_value"][labelled].any()
        assert (tr["outcomes"][labelled] == nat.SOLVE_NONE).all() and not tr["proven"][labelled].any()
    if "tb" in pols:  # (the full-inventory boards are no state of either table: a table side moves at random there)
        assert nat.HOW_TABLE in hows and nat.HOW_TABLE_SAMPLED in hows and nat.HOW_RANDOM in hows
    if "eval" in pols:
        assert nat.HOW_SEARCH in hows


def test_no_table_side_no_judge_is_collect_search_noise(cpu, deep):
    host, tb = deep
    st, tm, turn = H.start_boards(host, 6, 4, 2, seed=5)
    nets = (smoke_net(), ER.random_net(128, 77))
    keep = [k for k, _, _ in SOLVE_NAMES]
    for pols, its, deps, noise in ((("eval", "eval"), (6, 4), (2, 0), (64, 0)), (("random", "eval"), (0, 5), (0, 3), (0, 0)),
                                   (("random", "random"), (0, 0), (0, 0), (0, 0))):
        use = tuple(n if p == "eval" else None for n, p in zip(nets, pols))
        for layout, sample_plies, illegal_mode in (("time", 0, nat.ILLEGAL_NOOP), ("tile", 2, nat.ILLEGAL_TERMINATE)):
            exp = collect_solve(cpu.gbl_cpu_collect_search_noise, cpu.gbl_cpu_last_error, st, tm, turn, T, pols, use, its, deps, X, sample_plies,
                                illegal_mode, layout, SEED, ENV_BASE, PLY0, noise=noise)
            for table in (None, tb):  # (inventory / aux / table may be NULL, and are not read when given)
                same(H.host_collect_tb(table, st, tm, turn, T, pols, use, its, deps, noise, X, sample_plies, illegal_mode, layout, SEED,
                                       ENV_BASE, PLY0, None, 1, 600, keep), exp)


# ---- perfect play ------------------------------------------------------------------------------------------------------------------------
def test_perfect_play_ends_on_time(cpu, deep):
    """Table against table, the shortest wins and the longest losses: from a position of value V != 0 the game ends at exactly ply |V|
    and sign(V) is the starting mover's result; a position of value 0 is still running after 45 plies.  No exclusions."""
    host, tb = deep
    idx = np.random.default_rng(1).integers(0, host.positions, 20000)
    V = tb.table[idx].astype(np.int64)
    idx, V = idx[V != nat.TB_TERMINAL], V[V != nat.TB_TERMINAL]
    assert len(idx) == 15743 and (V != 0).sum() == 14900 and np.abs(V).max() == 36
    st = host.position(idx)
    n, plies = len(idx), 45
    tr, *_ = H.host_collect_tb(tb, st, np.zeros(n, np.int8), None, plies, ("tb", "tb"), mode=1, keep=["done", "winner", "how", "tb_value"])
    assert np.array_equal(tr["tb_value"][0], V)
    done = tr["done"] != 0
    first = np.where(done.any(0), done.argmax(0), plies)  # the ply index of the first game end, `plies` where there is none
    decided = V != 0
    assert np.array_equal(first[decided] + 1, np.abs(V[decided]))
    assert (first[~decided] == plies).all() and (~decided).sum() == 843
    ends = tr["winner"][first[decided], np.flatnonzero(decided)]
    assert np.array_equal(ends, np.sign(V[decided]))  # (the starting mover is player_1: winner +1 is its win)
    assert (tr["how"][0] == nat.HOW_TABLE).all()
    # the empty board is a draw
    e, *_ = H.host_collect_tb(tb, np.zeros((1, 27), np.int8), np.zeros(1, np.int8), None, plies, ("tb", "tb"), mode=1, keep=["done", "tb_value"])
    assert not e["done"].any() and not e["tb_value"].any()


def test_cross_pin_with_tb_targets_and_the_visits_sum(cpu, deep, wide):
    """gbl_cpu_tb_targets on cell t - 1's observation and mask rows (the position before ply t) reproduces a TABLEBASE ply's visits row
    and sign(tb_value); the row's sum is tb_count * |O|."""
    for (host, tb), pols in ((deep, ("tb", "tb")), (wide, ("tb", "random")), (deep, ("random", "tb"))):
        st, tm, turn = H.start_boards(host, 40, 10, 6, seed=29)
        for mode, count, sample_plies in ((0, 1, 0), (1, 600, 2), (0, 37, 2)):
            tr, *_ = H.host_collect_tb(tb, st, tm, turn, 6, pols, sample_plies=sample_plies, seed=SEED, mode=mode, count=count)
            labelled = np.isin(tr["how"], TABLE_HOWS)
            assert labelled[1:].sum() >= 50
            O = np.stack([[TR.targets(tr["tb_outcomes"][t, b][None], tr["tb_value"][t, b:b + 1], np.zeros(1), mode, 1)["visits"][0]
                           for b in range(len(st))] for t in range(6)])
            assert np.array_equal(tr["visits"][labelled], count * O[labelled])
            assert np.array_equal(tr["visits"].astype(np.int64).sum(-1)[labelled], count * O.sum(-1)[labelled])
            assert np.array_equal(tr["value"][labelled], np.sign(tr["tb_value"][labelled].astype(np.int64)) * 128 * count * O.sum(-1)[labelled])
            assert not tr["visits"][~labelled].any()
            t_, b_ = np.nonzero(labelled[1:])
            obs = np.ascontiguousarray(tr["observation"][t_, b_])
            mask = np.ascontiguousarray(tr["action_mask"][t_, b_])
            n = len(obs)
            v, z = np.full((n, 54), -7, np.int16), np.full(n, -7, np.int8)
            rc = cpu.gbl_cpu_tb_targets(tb.inv, tb.aux.ctypes.data, tb.table.ctypes.data, obs.ctypes.data, 117, mask.ctypes.data, 54, None,
                                        v.ctypes.data, 54, None, z.ctypes.data, 1, mode, count, None, None, None, n, None)
            assert rc == 0, cpu.gbl_cpu_last_error()
            assert np.array_equal(v, tr["visits"][1:][t_, b_]) and np.array_equal(z, np.sign(tr["tb_value"][1:][t_, b_]))


def test_sampling_plays_different_games_inside_O(cpu, deep):
    host, tb = deep
    n, plies = 64, 8
    st, tm, turn = np.zeros((n, 27), np.int8), np.zeros(n, np.int8), np.zeros(n, np.int32)
    plain, *_ = H.host_collect_tb(tb, st, tm, turn, plies, ("tb", "tb"), sample_plies=0, seed=3)
    assert len({tuple(r) for r in plain["actions"].T}) == 1  # nothing is drawn: one game, n times
    for mode in (0, 1):
        tr, *_ = H.host_collect_tb(tb, st, tm, turn, plies, ("tb", "tb"), sample_plies=6, seed=3, mode=mode, count=5)
        assert len({tuple(r) for r in tr["actions"].T}) > 1
        sampled = tr["how"] == nat.HOW_TABLE_SAMPLED
        assert sampled[:6].all() and (tr["how"][6:] == nat.HOW_TABLE).all()
        t_, b_ = np.nonzero(sampled)
        assert (tr["visits"][t_, b_, tr["actions"][t_, b_]] == 5).all()  # every sampled action lies in O
        assert (np.sign(tr["tb_played"][sampled]) == np.sign(tr["tb_value"][sampled])).all()  # ... so it keeps the result: a draw
        assert not tr["tb_value"].any()


def test_every_optional_pointer_null_in_turn(cpu, deep):
    host, tb = deep
    st, tm, turn = H.start_boards(host, 8, 3, 2, seed=41)
    net = smoke_net()
    args = dict(nets=(net, None), its=(4, 0), deps=(2, 0), noise=(32, 0), sample_plies=2, seed=SEED, count=3)
    full = H.host_collect_tb(tb, st, tm, turn, 4, ("eval", "tb"), **args)
    names = [k for k, _, _ in H.TB_NAMES]
    for drop in names:
        keep = [k for k in names if k != drop]
        got = H.host_collect_tb(tb, st, tm, turn, 4, ("eval", "tb"), keep=keep, **args)
        same(got, ({k: full[0][k] for k in keep},) + full[1:])
    # no turn counter (sample_plies 0) and the tallies
    counters = np.zeros(nat.COUNTER_STRIPES * nat.COUNTER_STRIDE, np.int64)
    a = H.host_collect_tb(tb, st, tm, None, 4, ("tb", "random"), seed=SEED, counters=counters, keep=["done", "actions"])
    assert a[4] is None and counters.sum() > 0


# ---- the recorded argument errors -----------------------------------------------------------------------------------------------------
def replay(table, flavours):
    """tests/golden/selfplay_tb_arg_errors.json: search_harness's format, an argument "inv" being the case's "inventory" as an int32[3]
    on the host (the library reads it at the call; null: NULL)."""
    for c in table:
        inv = None if c["inventory"] is None else TH.inv_array(c["inventory"])  # (alive until the case has been replayed)
        where = None if inv is None else C.addressof(inv)
        replay_arg_errors([dict(c, args=[where if x == "inv" else x for x in c["args"]])], flavours)


def test_argument_errors_replay_the_recorded_table(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "selfplay_tb_arg_errors.json")))
    assert len(table) >= 20 and {c["fn"] for c in table} == {"collect_search_tb"}
    replay(table, ("device", "host"))  # (the device entry point checks its arguments before any HIP call: no GPU needed)


# ---- the Python surface and Tablebase.judge ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tb_small():
    tb = G.Tablebase((1, 1, 1), "cpu")
    tb.build()
    assert tb.complete
    return tb


def test_python_surface_on_cpu(cpu, tb_small, deep):
    def fresh():
        return G.BatchedGobblet(65, "cpu", auto_reset=True, seed=11, track_turn=True)
    assert G.BatchedGobblet.POLICIES["tablebase"] == nat.POLICY_TABLEBASE == 6 and (nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED) == (6, 7)
    env = fresh()
    traj = env.collect(6, policies=("tablebase", "random"), search=dict(tablebase=tb_small, tb_mode="shortest", tb_count=7, judge=True,
                                                                        sample_plies=2))
    assert traj["tb_outcomes"].shape == (6, 65, 54) and traj["tb_value"].dtype == torch.int8 and traj["tb_played"].shape == (6, 65)
    tab = H.Table((1, 1, 1), tb_small._aux.numpy(), tb_small.table.numpy())
    z = np.zeros(65, np.int8)
    exp = H.host_collect_tb(tab, np.zeros((65, 27), np.int8), z, np.zeros(65, np.int32), 6, ("tb", "random"), sample_plies=2, seed=11, mode=1, count=7)
    for k in exp[0]:
        if k not in ("outcomes", "proven"):  # (no guard was asked for: the wrapper made no solver arrays)
            assert np.array_equal(traj[k].numpy().reshape(exp[0][k].shape), exp[0][k]), k
    assert "outcomes" not in traj
    how = set(traj["how"].numpy().ravel().tolist())
    assert {nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED, nat.HOW_RANDOM} <= how  # (player_2 soon plays a piece (1, 1, 1) lacks)
    # a policy instance supplies its table; the tile layout; no judge: no judge arrays
    pol = G.TablebaseGobbletPolicy(tb_small)
    t2 = fresh().collect(3, policies=(pol, pol), layout="tile")
    assert "tb_value" not in t2 and t2["visits"].shape == (2, 3, 64, 54)
    assert (t2["how"][0] == nat.HOW_TABLE).all() and (t2["how"][1, :, :1] == nat.HOW_TABLE).all()  # (65 boards: one in the last tile)
    # the judge beside an evaluator window; outcome_targets and training_batch take the window as it is
    net = smoke_net()
    ev = G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, 1, 9, 9, device="cpu")
    e3 = fresh()
    t3 = e3.collect(4, policies=("evaluator", "tablebase"), search=dict(evaluator=ev, iterations=4, tablebase=tb_small, judge=True, tb_count=9))
    census = tb_small.judge(t3)
    assert set(census) == {"player_1", "player_2"} and sum(sum(v.values()) for v in census.values()) == 4 * 65
    assert t3["z_exact"].shape == t3["regret"].shape == (4, 65)
    # outcome_targets and training_batch take a window as it is: from won positions of the (2, 2, 0) table the games end inside it,
    # and a table ply's row is kept with its sum, tb_count * |O|
    host, raw = deep
    big = G.Tablebase(DEEP, "cpu")
    big.table.copy_(torch.from_numpy(raw.table))
    big.sweeps, big.complete = 40, True
    idx = np.random.default_rng(2).integers(0, host.positions, 4000)
    idx = idx[(raw.table[idx] >= 1) & (raw.table[idx] <= 5)][:65]
    e4 = fresh()
    sd = e4.state_dict()
    sd["squares"] = torch.from_numpy(host.position(idx))
    e4.load_state_dict(sd)
    t4 = e4.collect(8, policies=("tablebase", "tablebase"), search=dict(tablebase=big, tb_mode="shortest", tb_count=9, judge=True))
    assert big.judge(t4)["player_1"]["kept"] > 0 and not (t4["regret"] > 0).any()  # (perfect play throws nothing away)
    e4.outcome_targets(t4)
    batch = e4.training_batch(t4, 256, call=1)
    idx4 = batch["index"].numpy()
    ok = idx4[:, 0] >= 0
    cell = (idx4[ok, 0], idx4[ok, 1])
    rows = batch["visits"].numpy()[ok].astype(np.int64)
    O = (t4["tb_outcomes"].numpy()[cell] == t4["tb_value"].numpy()[cell][:, None]).sum(1)
    assert ok.sum() >= 100 and (t4["how"].numpy()[cell] == nat.HOW_TABLE).all() and (O > 0).all() and (rows.sum(1) == 9 * O).all()
    assert np.array_equal(batch["z"].numpy()[ok], t4["z_exact"].numpy()[cell])  # the game's result is the table's
    # existing calls keep their entry points; what the wrapper refuses
    t5 = fresh().collect(2, policies=("evaluator", "random"), search=dict(evaluator=ev, iterations=2))
    assert "tb_value" not in t5
    half = G.Tablebase((1, 1, 0), "cpu")
    half.build(max_sweeps=1)
    assert not half.complete
    with pytest.raises(ValueError, match="not complete"):
        fresh().collect(2, policies=("tablebase", "random"), search=dict(tablebase=half))
    fresh().collect(2, policies=("tablebase", "random"), search=dict(tablebase=half, allow_incomplete=True))
    for bad in (dict(), dict(tablebase=tb_small, tb_mode="best"), dict(tablebase=tb_small, tb_count=601), dict(tablebase=tb_small, bogus=1)):
        with pytest.raises(ValueError):
            fresh().collect(2, policies=("tablebase", "random"), search=bad)
    with pytest.raises(ValueError):
        fresh().collect(2, policies=("tablebase", "greedy"), search=dict(tablebase=tb_small))
    with pytest.raises(ValueError):
        env.trajectory_buffers(3, search_outputs=True, tablebase_outputs=True)


def test_judge_on_a_hand_made_trajectory(tb_small):
    """Every regret class, on both sides: (tb_value, tb_played, row all NONE) -> (z_exact, regret)."""
    N_ = nat.SOLVE_NONE
    rows = [(5, 3, False, 1, 0), (5, 0, False, 1, 1), (5, -4, False, 1, 2), (0, 0, False, 0, 0), (0, -2, False, 0, 3), (-6, -6, False, -1, 0),
            (-6, -2, False, -1, 0), (0, N_, True, nat.Z_OPEN, -1), (3, N_, False, 1, -1), (1, 1, False, 1, 0)]
    n = len(rows)
    traj = {"tb_value": torch.tensor([[r[0] for r in rows]] * 2, dtype=torch.int8), "tb_played": torch.tensor([[r[1] for r in rows]] * 2, dtype=torch.int8),
            "tb_outcomes": torch.zeros((2, n, 54), dtype=torch.int8), "mover": torch.tensor([[0] * n, [1] * n], dtype=torch.int8)}
    for b, r in enumerate(rows):
        if r[2]:
            traj["tb_outcomes"][:, b] = N_
    census = tb_small.judge(traj)
    assert traj["z_exact"].dtype == torch.int8 and traj["regret"].dtype == torch.int8
    assert traj["z_exact"].tolist() == [[r[3] for r in rows]] * 2 and traj["regret"].tolist() == [[r[4] for r in rows]] * 2
    want = {"kept": 5, "win_to_draw": 1, "win_to_loss": 1, "draw_to_loss": 1, "no_verdict": 2}
    assert census == {"player_1": want, "player_2": want}
