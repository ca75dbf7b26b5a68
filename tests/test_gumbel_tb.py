"""gbl_collect_gumbel_tb on the host flavour (no GPU): Gumbel self-play with the exact table as a third policy and as the judge of
every ply.  Against the ply-by-ply loop on the host flavour's own entry points (gbl_cpu_tb_probe -> the table's pick, or
gbl_cpu_tree_search_gumbel(call = q) / gbl_cpu_tree_search_eval -> gbl_cpu_step_into) with every branch counted; against a Python
restatement composed from tests/selfplay_tb_restatement.py and tests/gumbel_restatement.py; the two identities (no table side and no
judge array: gbl_cpu_collect_search_gumbel; both considered 0: gbl_cpu_collect_search_tb at depths and noise 0), a split window, two
shards, *ply_dev and the counters; tb_played read off the trajectory alone; the consumers; the argument errors of both flavours in
the header's order; the declaration in both headers against the table in _native.py; and collect()'s spelling.

Boards: tests/selfplay_tb_harness.py's start_boards on the complete (2, 2, 0) table -- positions of the inventory, full-inventory
boards outside it (a table side moves at random there, the verdict row is GBL_SOLVE_NONE) and fresh boards.  Networks: smoke()'s
seeded integer evaluator (H = 64) and a second one of 128 hidden units."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests import selfplay_tb_harness as TBH
from tests import tablebase_harness as TH
from tests.gumbel_harness import host_collect_gumbel
from tests.gumbel_tb_harness import (BRANCHES, CASES, ENTRY, EXPLORE, INVENTORY, JUDGE, SHARED, boards, call_args, composed_loop,
                                     host_collect_gtb, judge_keep, restate_collect_gtb)
from tests.selfplay_harness import _evaluator, same
from tests.test_gumbel_search import Counting
from tests.test_selfplay_solve import smoke_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, ENV_BASE, PLY0, T = 0xFEDCBA9876543210, (1 << 41) + 77, 3, 6


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(8)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.fixture(scope="module")
def world(cpu):
    """The complete (2, 2, 0) table, built once: (host, Table)."""
    host = TH.Host(INVENTORY)
    table, counts = host.build()
    assert counts[-1] == 0
    return host, TBH.Table(INVENTORY, host.aux, table)


@pytest.fixture(scope="module")
def start(world):
    return boards(world[0], 130)


@pytest.fixture(scope="module")
def nets():
    return {64: smoke_net(), 128: R.random_net(128, 77)}


# (case, layout, sample_plies, gumbel_noise, scale, hidden, illegal_mode, tb_mode, tb_count): every case in both layouts, with noise
# 0 / 1, scale 0 / 23, both illegal modes and both table modes; case 0 with sample_plies 0 and 2
LOOPS = [(0, "time", 0, 1, 23, 64, nat.ILLEGAL_NOOP, 0, 1), (0, "tile", 2, 0, 0, 128, nat.ILLEGAL_TERMINATE, 1, 7),
         (0, "time", 2, 1, 23, 64, nat.ILLEGAL_NOOP, 1, 600), (0, "tile", 0, 0, 0, 64, nat.ILLEGAL_TERMINATE, 0, 3),
         (1, "time", 0, 1, 23, 128, nat.ILLEGAL_NOOP, 0, 1), (1, "tile", 2, 0, 0, 64, nat.ILLEGAL_TERMINATE, 1, 7),
         (2, "time", 2, 1, 23, 64, nat.ILLEGAL_NOOP, 0, 1), (2, "tile", 0, 0, 0, 128, nat.ILLEGAL_TERMINATE, 1, 7),
         (3, "time", 0, 1, 23, 128, nat.ILLEGAL_NOOP, 0, 1), (3, "tile", 0, 0, 0, 64, nat.ILLEGAL_TERMINATE, 1, 7),
         (4, "time", 0, 1, 23, 64, nat.ILLEGAL_NOOP, 0, 1), (4, "tile", 2, 0, 0, 64, nat.ILLEGAL_TERMINATE, 1, 7),
         (5, "time", 0, 1, 23, 64, nat.ILLEGAL_NOOP, 0, 1), (5, "tile", 2, 0, 0, 64, nat.ILLEGAL_TERMINATE, 1, 7)]
# the branches a case must meet on 65 boards x 6 plies (BRANCHES' names), whatever the run; "how 7" where the run samples
KEEPS, LOSES, KEYS, HOW6, HOW7, RANDOM, NONE_ROW = BRANCHES
MEETS = {0: (KEEPS, LOSES, HOW6, RANDOM, NONE_ROW), 1: (HOW6, RANDOM), 2: (KEEPS, LOSES, KEYS, NONE_ROW), 3: (KEEPS, LOSES, NONE_ROW),
         4: (HOW6, RANDOM, NONE_ROW), 5: (HOW6, RANDOM)}


@pytest.mark.parametrize("case,layout,sample_plies,noise,scale,hidden,illegal_mode,mode,count", LOOPS)
def test_host_flavour_equals_the_ply_by_ply_loop(cpu, world, start, nets, case, layout, sample_plies, noise, scale, hidden, illegal_mode, mode,
                                                 count):
    host, tb = world
    pols, considered, its, judge = CASES[case]
    st, tm, turn = (x[:65] for x in start)
    net = nets[hidden]
    use = tuple(net if p == "eval" else None for p in pols)
    got = host_collect_gtb(tb, st, tm, turn, T, pols, use, its, considered, noise, 50, scale, EXPLORE, sample_plies, illegal_mode, layout, SEED,
                           ENV_BASE, PLY0, mode=mode, count=count, keep=judge_keep(judge))
    *exp, met = composed_loop(cpu, host, tb, st, tm, turn, T, pols, (net, net), its, considered, noise, 50, scale, EXPLORE, sample_plies,
                              illegal_mode, SEED, ENV_BASE, PLY0, mode, count, judge)
    assert set(got[0]) == set(SHARED) | (set(JUDGE) if judge else set()) and len(got[0]) == (17 if judge else 14)
    same(got, exp)
    print("case %d: %s" % (case, met))
    need = MEETS[case] + ((HOW7,) if sample_plies and "tb" in pols else ())
    assert all(met[k] > 0 for k in need), met
    how = got[0]["how"]
    assert set(np.unique(how).tolist()) <= {nat.HOW_RANDOM, nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED, nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED,
                                            nat.HOW_GUMBEL}
    if case == 2:  # the PUCT side honours sample_plies, the Gumbel side does not read it
        assert ((how == nat.HOW_SEARCH_SAMPLED).any()) == bool(sample_plies)
    table_plies = np.isin(how, (nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED))
    tr = got[0]
    assert not tr["priors"][table_plies].any() and not tr["nodes"][table_plies].any() and not tr["root_value"][table_plies].any()


def test_every_branch_occurs_in_the_reference_loop(cpu, world, start, nets):
    """The seven branches of the issue, counted by the composed loop alone over the cases' first runs."""
    host, tb = world
    st, tm, turn = (x[:65] for x in start)
    total = dict.fromkeys(BRANCHES, 0)
    for case, sample_plies in ((0, 2), (2, 0)):
        pols, considered, its, judge = CASES[case]
        net = nets[64]
        met = composed_loop(cpu, host, tb, st, tm, turn, T, pols, (net, net), its, considered, 1, 50, 23, EXPLORE, sample_plies, nat.ILLEGAL_NOOP,
                            SEED, ENV_BASE, PLY0, 0, 1, judge)[-1]
        for k, v in met.items():
            total[k] += v
    print(total)
    assert all(v > 0 for v in total.values()), total


def small_boards(start):
    """8 boards for the Python restatement: the first six of the mix and two fresh ones, some inside the sampled plies."""
    st = np.concatenate([start[0][:6], np.zeros((2, 27), np.int8)])
    tm = np.concatenate([start[1][:6], np.zeros(2, np.int8)])
    turn = np.concatenate([start[2][:6] % 4, np.zeros(2, np.int32)])
    return st, tm, turn


@pytest.mark.parametrize("illegal_mode", [nat.ILLEGAL_NOOP, nat.ILLEGAL_TERMINATE])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_flavour_equals_restatement(cpu, world, start, nets, case, illegal_mode):
    host, tb = world
    pols, considered, its, judge = CASES[case]
    its = tuple(min(x, 8) for x in its)  # (the restatement walks its trees in Python)
    st, tm, turn = small_boards(start)
    net = nets[64]
    use = tuple(net if p == "eval" else None for p in pols)
    mode, count = case % 2, 1 + 5 * case
    exp = restate_collect_gtb(lambda s, m: host.probe(tb.table, s, m), st, tm, turn, 4, pols, (net, net), its, considered, 1, 50, 23, EXPLORE, 2,
                              illegal_mode, 9, (1 << 40) - 20, 8, mode, count, judge)
    for layout, ply_dev in (("time", None), ("tile", 3)):
        got = host_collect_gtb(tb, st, tm, turn, 4, pols, use, its, considered, 1, 50, 23, EXPLORE, 2, illegal_mode, layout, 9, (1 << 40) - 20,
                               8 - (ply_dev or 0), ply_dev=ply_dev, mode=mode, count=count, keep=judge_keep(judge))
        same(got, exp)


def test_identities(cpu, world, start, nets):
    host, tb = world
    st, tm, turn = (x[:65] for x in start)
    pair = (nets[64], nets[128])
    for layout in ("time", "tile"):
        # no TABLEBASE side, the three judge arrays NULL: every array is gbl_cpu_collect_search_gumbel's; the table may be NULL, and its
        # mode and count are then not read either
        exp = host_collect_gumbel(st, tm, turn, T, ("eval", "eval"), pair, (8, 16), (16, 0), 1, 50, 23, EXPLORE, 3, nat.ILLEGAL_NOOP, layout, SEED,
                                  ENV_BASE, PLY0)
        for table, mode, count in ((None, 77, -5), (tb, 0, 1)):
            same(host_collect_gtb(table, st, tm, turn, T, ("eval", "eval"), pair, (8, 16), (16, 0), 1, 50, 23, EXPLORE, 3, nat.ILLEGAL_NOOP, layout,
                                  SEED, ENV_BASE, PLY0, mode=mode, count=count, keep=list(SHARED)), exp)
        # both considered 0: every shared array is gbl_cpu_collect_search_tb's at depths (0, 0) and noise (0, 0), whatever the rule's three say
        for pols, use, its in ((("eval", "tb"), (pair[0], None), (8, 0)), (("eval", "eval"), pair, (8, 16)), (("tb", "random"), (None, None), (0, 0))):
            got = host_collect_gtb(tb, st, tm, turn, T, pols, use, its, (0, 0), 5, -3, 999, EXPLORE, 3, nat.ILLEGAL_TERMINATE, layout, SEED,
                                   ENV_BASE, PLY0, mode=1, count=9)
            exp = TBH.host_collect_tb(tb, st, tm, turn, T, pols, use, its, (0, 0), (0, 0), EXPLORE, 3, nat.ILLEGAL_TERMINATE, layout, SEED,
                                      ENV_BASE, PLY0, None, 1, 9)
            assert (exp[0].pop("outcomes") == nat.SOLVE_NONE).all() and (exp[0].pop("proven") == 0).all()
            same(got, exp)
    # a RANDOM / TABLEBASE side's considered, iterations and evaluator are not read
    got = host_collect_gtb(tb, st, tm, turn, T, ("tb", "eval"), (None, pair[1]), (-9, 8), (99, 4), seed=SEED, ply0=PLY0, sample_plies=2)
    same(got, host_collect_gtb(tb, st, tm, turn, T, ("tb", "eval"), (None, pair[1]), (0, 8), (0, 4), seed=SEED, ply0=PLY0, sample_plies=2))


def test_split_window_shards_ply_dev_and_counters(cpu, world, start, nets):
    host, tb = world
    st, tm, turn = start
    args = (("eval", "tb"), (nets[64], None), (8, 0), (16, 0))
    kw = dict(sample_plies=2, seed=SEED, mode=1, count=3)
    whole = host_collect_gtb(tb, st, tm, turn, T, *args, ply0=PLY0, **kw)
    # two shards through env_base
    halves = [host_collect_gtb(tb, st[a:b], tm[a:b], turn[a:b], T, *args, env_base=a, ply0=PLY0, **kw) for a, b in ((0, 65), (65, 130))]
    for k, v in whole[0].items():
        assert np.array_equal(v, np.concatenate([h[0][k] for h in halves], axis=1)), k
    for i in (1, 2, 3, 4):
        assert np.array_equal(whole[i], np.concatenate([h[i] for h in halves]))
    # the window in two calls through ply0: the second goes on from the first's boards and turn counters
    first = host_collect_gtb(tb, st, tm, turn, 2, *args, ply0=PLY0, **kw)
    second = host_collect_gtb(tb, first[1], first[2], first[4], T - 2, *args, ply0=PLY0 + 2, **kw)
    for k, v in whole[0].items():
        assert np.array_equal(v, np.concatenate([first[0][k], second[0][k]])), k
    for i in (1, 2, 4):
        assert np.array_equal(whole[i], second[i])
    # *ply_dev
    same(host_collect_gtb(tb, st, tm, turn, T, *args, ply0=0, ply_dev=PLY0, **kw), whole)
    other = host_collect_gtb(tb, st, tm, turn, T, *args, ply0=PLY0 + 1, **kw)
    assert not np.array_equal(other[0]["visits"], whole[0]["visits"])  # (the Gumbel row moves with the ply index)
    # counters: the plies and the finished games of the window
    counters = np.zeros(nat.COUNTER_STRIPES * nat.COUNTER_STRIDE, np.int64)
    got = host_collect_gtb(tb, st, tm, turn, T, *args, ply0=PLY0, counters=counters, **kw)
    same(got, whole)
    tally = counters.reshape(nat.COUNTER_STRIPES, nat.COUNTER_STRIDE).sum(0)
    assert tally[0] == 130 * T and tally[1] == whole[0]["done"].sum()


def test_tb_played_is_the_outcome_of_the_action(cpu, world, start, nets):
    """Off the trajectory alone: tb_played[cell] == tb_outcomes[cell][action], GBL_SOLVE_NONE where the action is -1; tb_value is the
    best byte of the row by the probe's key; and a Gumbel ply's target bytes lie exactly on the legal actions."""
    host, tb = world
    st, tm, turn = start
    for case in (0, 2, 3):
        pols, considered, its, judge = CASES[case]
        use = tuple(nets[64] if p == "eval" else None for p in pols)
        tr = host_collect_gtb(tb, st, tm, turn, 8, pols, use, its, considered, sample_plies=2, seed=5, mode=case % 2, count=2)[0]
        out, played, act, how = tr["tb_outcomes"], tr["tb_played"], tr["actions"], tr["how"]
        t_, b_ = np.nonzero(act >= 0)
        assert np.array_equal(played[t_, b_], out[t_, b_, act[t_, b_]])
        assert (played[act < 0] == nat.SOLVE_NONE).all()
        rule = how == nat.HOW_GUMBEL
        assert rule.sum() > 100 and (played[rule] != nat.SOLVE_NONE).sum() >= 10  # (the property was put to the test on judged rule plies)
        empty = (out == nat.SOLVE_NONE).all(-1)
        assert empty.any() and not tr["tb_value"][empty].any()
        # the position before ply t + 1 is cell t's: a Gumbel ply's row is 1 .. 255 exactly on its legal mask
        later = rule[1:]
        rows, masks = tr["visits"][1:][later], tr["action_mask"][:-1][later]
        assert ((rows >= 1) & (rows <= 255))[masks != 0].all() and not rows[masks == 0].any()


def python_table(world):
    host, raw = world
    big = G.Tablebase(INVENTORY, "cpu")
    big.table.copy_(torch.from_numpy(raw.table))
    big.sweeps, big.complete = 40, True
    assert np.array_equal(big._aux.numpy(), host.aux)
    return big


def positions_env(world, start, n, seed=11):
    """An environment on the first n start boards."""
    env = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, env_base=3, track_turn=True)
    sd = env.state_dict()
    sd["squares"], sd["to_move"], sd["turn"] = (torch.from_numpy(np.ascontiguousarray(x[:n])) for x in start)
    env.load_state_dict(sd)
    return env


def test_the_consumers_take_the_window_unchanged(cpu, world, start, nets):
    n, plies, its = 130, 12, 16
    big = python_table(world)
    ev = _evaluator(nets[64])
    env = positions_env(world, start, n)
    tr = env.collect(plies, policies=("tablebase", "evaluator"), out="fresh",
                     search=dict(evaluator=ev, iterations=its, explore=EXPLORE, sample_plies=2,
                                 gumbel=dict(considered=16, tablebase=big, tb_mode="result", tb_count=4, judge=True)))
    assert {"tb_outcomes", "tb_value", "tb_played"} <= set(tr) and "outcomes" not in tr
    census = big.judge(tr)
    assert set(census) == {"player_1", "player_2"} and sum(sum(v.values()) for v in census.values()) == plies * n
    lost = sum(census["player_2"][k] for k in ("win_to_draw", "win_to_loss", "draw_to_loss"))
    assert lost > 0 and census["player_2"]["kept"] > 0  # (an untrained Gumbel-16 side throws results away)
    assert not any(census["player_1"][k] for k in ("win_to_draw", "win_to_loss", "draw_to_loss"))  # (the table never does)
    env.outcome_targets(tr)
    how, z, done = tr["how"].numpy(), tr["z"].numpy(), tr["done"].numpy()
    assert set(np.unique(how).tolist()) == {nat.HOW_RANDOM, nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED, nat.HOW_GUMBEL}
    valid = np.zeros_like(how, bool)
    valid[1:] = (z[1:] != nat.Z_OPEN) & (done[:-1] == 0)
    keep = valid & np.isin(how, (nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED, nat.HOW_GUMBEL))  # the kept rows: the valid cells with how 6, 7 or 10
    K = int(keep.sum())
    assert (keep & (how == nat.HOW_GUMBEL)).sum() > 20 and (keep & (how == nat.HOW_TABLE)).sum() > 5  # (both kinds were put to the test)
    rows = tr["visits"].numpy()
    assert (rows[how == nat.HOW_GUMBEL].sum(1) >= 255).all() and not rows[how == nat.HOW_RANDOM].any()
    # regret-driven priorities: a ply that threw a result away weighs more
    weights = torch.tensor([1, 1, 4, 8, 8], dtype=torch.int32)  # (regret -1, 0, 1, 2, 3)
    buf = G.ReplayBuffer(2048, "cpu", prioritized=True)
    buf.append(env, tr, tag=3, priority=weights[tr["regret"].long() + 1])
    assert buf.total == K
    at = np.argwhere(keep)
    tt, bb = at[:, 0], at[:, 1]
    assert np.array_equal(buf.visits[:K].numpy(), rows[tt, bb]) and np.array_equal(buf.z[:K].numpy(), z[tt, bb])
    assert np.array_equal(buf.priority[:K].numpy(), weights.numpy()[tr["regret"].numpy().astype(np.int64)[tt, bb] + 1])
    drawn = buf.batch(256, symmetries=None, call=1, seed=5, prioritized=True)
    slot = drawn["index"][:, 0].numpy()
    assert (slot >= 0).all() and np.array_equal(drawn["visits"].numpy(), rows[tt[slot], bb[slot]])
    trainer = G.GobbletTrainer(64, "cpu", seed=1)
    stats = trainer.step(drawn)
    assert int(stats[2]) == 256 and np.isfinite(stats.numpy()).all() and float(stats[0]) > 0.0
    fit = buf.fit(trainer, 2, batch=128, symmetries=None, seed=3)
    assert fit.shape == (2, 4) and np.isfinite(fit.numpy()).all()
    tb_ = env.training_batch(tr, 256, symmetries=None, call=2)
    t_, b_ = tb_["index"][:, 0].numpy(), tb_["index"][:, 1].numpy()
    ok = t_ >= 0
    assert ok.sum() > 64 and keep[t_[ok], b_[ok]].all()
    seen = how[t_[ok], b_[ok]]
    assert (seen == nat.HOW_TABLE).any() and (seen == nat.HOW_GUMBEL).any()


CONSIDERED_MSG = b"considered0 / considered1 must be in [0, 54]"
POLICY_MSG = b"policy0 / policy1: GBL_POLICY_RANDOM, GBL_POLICY_EVAL_TREE or GBL_POLICY_TABLEBASE"
MODE_MSG = b"tb_mode must be GBL_TB_TARGET_RESULT or GBL_TB_TARGET_SHORTEST"
COUNT_MSG = b"tb_count must be in [1, 600]"
ERRORS = [  # (name, overrides, message or None: GBL_OK), in the header's order
    ("n < 0 before all", dict(n=-1, illegal_mode=7, considered=(55, 0)), b"n < 0"),
    ("the illegal mode", dict(illegal_mode=7, pols=(2, "eval")), b"illegal_mode must be GBL_ILLEGAL_NOOP or GBL_ILLEGAL_TERMINATE"),
    ("a policy outside the three", dict(pols=(nat.POLICY_TREE, "eval"), its=(0, 5), mode=7), POLICY_MSG),
    ("a policy outside the three, the other side", dict(pols=("tb", 9)), POLICY_MSG),
    ("an evaluator before the table", dict(evs=(False, True), mode=7), b"ev must not be NULL"),
    ("iterations before the table", dict(its=(0, 5), mode=7, considered=(55, 4)), b"iterations must be in [1, 512]"),
    ("the window before the table", dict(sample_plies=-1, mode=7), b"sample_plies < 0"),
    ("tb_mode", dict(mode=2, count=0, inv=None, considered=(55, 4)), MODE_MSG),
    ("tb_mode, read for a table side without a judge array", dict(pols=("eval", "tb"), judge=False, mode=-1), MODE_MSG),
    ("tb_count 0", dict(count=0, inv=None, considered=(55, 4)), COUNT_MSG),
    ("tb_count 601", dict(count=601), COUNT_MSG),
    ("the inventory missing", dict(inv=None, considered=(55, 4)), b"inventory must not be NULL"),
    ("an inventory entry of 3", dict(inv=(2, 3, 0), considered=(55, 4)), b"inventory entries must be in [0, 2]"),
    ("considered 55", dict(considered=(55, 4), noise=2, vo=256, scale=65), CONSIDERED_MSG),
    ("considered -1", dict(considered=(16, -1), n=1), CONSIDERED_MSG),
    ("gumbel_noise 2", dict(noise=2, vo=256, scale=65), b"gumbel_noise must be 0 or 1"),
    ("visit_offset 256", dict(vo=256, scale=65), b"visit_offset must be in [0, 255]"),
    ("scale 65", dict(scale=65, n=1), b"scale must be in [0, 64]"),
    ("state", dict(n=1), b"state must not be NULL"),
    ("to_move", dict(n=1, state=True), b"to_move must not be NULL"),
    ("done", dict(n=1, state=True, to_move=True), b"done must not be NULL"),
    ("aux after the boards", dict(n=1, state=True, to_move=True, done=True, aux=False, table=False), b"aux must not be NULL"),
    ("table after aux", dict(n=1, state=True, to_move=True, done=True, table=False), b"table must not be NULL"),
    ("an evaluator's pointers last", dict(n=1, state=True, to_move=True, done=True, empty_net=True), b"the evaluator's w1 / b1 / w2 / b2 must not be NULL"),
    ("nobody reads the table: its mode, count and pointers are not looked at",
     dict(judge=False, mode=9, count=0, inv=None, aux=False, table=False, n=1, state=True, to_move=True, done=True, plies=0), None),
    ("no Gumbel side reads the three", dict(considered=(0, 0), noise=2, vo=-1, scale=65), None),
    ("a TABLEBASE side's bad values are ignored", dict(pols=("tb", "eval"), its=(-4, 5), considered=(-5, 4), evs=(False, True)), None),
    ("a RANDOM side's too, nor do they make the three read", dict(pols=("eval", "random"), considered=(0, 9), its=(8, 9999), scale=99,
                                                                 evs=(True, False)), None),
    ("the ends of the ranges", dict(considered=(54, 1), noise=0, vo=255, scale=64, count=600, mode=1), None),
]


@pytest.mark.parametrize("flavour", ["host", "device"])
def test_argument_errors(flavour):
    """(the device entry point checks its arguments before any HIP call: no GPU needed)"""
    lib, prefix = (nat.cpu_raw(), "gbl_cpu_") if flavour == "host" else (nat.lib(), "gbl_")
    err, f = getattr(lib, prefix + "last_error"), getattr(lib, prefix + "collect_gumbel_tb")
    net = smoke_net()
    zeros = np.zeros((64, 64), np.int8)  # (boards, a judge array, aux and the table of the calls that stop before they read them)

    def ptr(a):
        return None if a is None else a.ctypes.data
    for name, over, msg in ERRORS:
        kw = dict(pols=("eval", "eval"), its=(8, 5), considered=(16, 4), noise=1, vo=50, scale=23, n=0, state=False, to_move=False, done=False,
                  evs=(True, True), judge=True, mode=0, count=1, inv=(2, 2, 0), aux=True, table=True, illegal_mode=nat.ILLEGAL_NOOP,
                  sample_plies=0, plies=4, empty_net=False)
        kw.update(over)
        evs = [net.struct() if e else None for e in kw["evs"]]
        if kw["empty_net"]:
            evs[0].w1 = None
        st, tm, dn = (zeros if kw[k] else None for k in ("state", "to_move", "done"))
        inv = None if kw["inv"] is None else TH.inv_array(kw["inv"])  # (alive until the call has returned)
        table3 = dict(inventory=inv, aux=ptr(zeros) if kw["aux"] else None, table=ptr(zeros) if kw["table"] else None)
        traj = {"tb_value": zeros} if kw["judge"] else {}
        rc = f(*call_args(ptr, st, tm, dn, traj, kw["n"], 64, 64, 1, 0, 0, None, kw["plies"], kw["pols"], 16, kw["sample_plies"],
                          kw["illegal_mode"], None, None, None, evs, kw["its"], kw["considered"], kw["noise"], kw["vo"], kw["scale"], table3,
                          kw["mode"], kw["count"]))
        if msg is None:
            assert rc == nat.OK, (name, err())
        else:
            assert rc == nat.ERR_ARG and err() == msg, (name, rc, err())


def test_aux_alignment_on_the_device_flavour():
    """aux 16-byte aligned where the call reads the table: GBL_ERR_ALIGN, after every GBL_ERR_ARG and before any HIP call; the host
    flavour takes the same call."""
    net = smoke_net()
    buf = np.zeros(4096 + 64, np.int8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    inv = TH.inv_array(INVENTORY)
    boards_ = np.zeros((64, 27), np.int8)

    def args(aux, n=1, plies=0):
        table3 = dict(inventory=inv, aux=aux, table=base)
        return call_args(lambda a: None if a is None else a.ctypes.data, boards_, boards_[:, 0].copy(), boards_[:, 1].copy(), {}, n, 64, 64, 1, 0, 0,
                         None, plies, ("eval", "tb"), 16, 0, nat.ILLEGAL_NOOP, None, None, None, [net.struct(), None], (8, 0), (16, 0), 1, 50, 23,
                         table3, 0, 1)
    assert nat.cpu_raw().gbl_cpu_collect_gumbel_tb(*args(base + 8)) == nat.OK  # (plies == 0: nothing to do)
    assert nat.lib().gbl_collect_gumbel_tb(*args(base)) == nat.OK
    rc = nat.lib().gbl_collect_gumbel_tb(*args(base + 8, plies=1))
    assert rc == nat.ERR_ALIGN and b"aux" in nat.lib().gbl_last_error(), (rc, nat.lib().gbl_last_error())


def test_the_table_is_both_headers_declaration():
    """nat.SELFPLAY_ARGS_TABLE against the declaration in include/gobblet_hip.h and include/gobblet_cpu.h, parameter by parameter: the
    name, and the ctype of its C type; and the arguments are gbl_collect_search_gumbel's up to and including `scale`, then
    gbl_collect_search_tb's table block in its order, before `stream`."""
    ctype_of = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}
    assert set(nat.SELFPLAY_ARGS_TABLE) == {ENTRY} and not set(nat.SELFPLAY_ARGS_TABLE) & (set(nat.SELFPLAY_ARGS) | set(nat.SELFPLAY_ARGS_MORE))
    assert not ENTRY.startswith("gbl_collect_search")
    table = nat.SELFPLAY_ARGS_TABLE[ENTRY]
    for header, name in (("gobblet_hip.h", ENTRY), ("gobblet_cpu.h", "gbl_cpu_" + ENTRY[4:])):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        declared = []
        for param in re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M).group(1).split(","):
            ctype, pointer, param_name = re.fullmatch(r"\s*(?:const )?(\w+) (\*?)(\w+)\s*", param).groups()
            declared.append((param_name, C.c_void_p if pointer else ctype_of[ctype]))
        assert declared == list(table), (header, [(d, t) for d, t in zip(declared, table) if d != t], len(declared), len(table))
    assert nat.SIGNATURES[ENTRY] == (C.c_int, [t for _, t in table]) == nat.CPU_SIGNATURES["gbl_cpu_" + ENTRY[4:]]
    gumbel, tb = nat.SELFPLAY_ARGS["gbl_collect_search_gumbel"], nat.SELFPLAY_ARGS["gbl_collect_search_tb"]
    assert table == gumbel[:-1] + tb[-9:] and table[-1][0] == "stream" and [k for k, _ in tb[-9:-1]] == [
        "inventory", "aux", "table", "tb_mode", "tb_count", "tb_outcome_traj", "tb_value_traj", "tb_played_traj"]
    assert nat.selfplay_table(ENTRY) is table and nat.selfplay_table("gbl_collect_gumbel_solve") is nat.SELFPLAY_ARGS_MORE["gbl_collect_gumbel_solve"]
    with pytest.raises(TypeError, match="'tb_count'"):
        nat.selfplay_args(ENTRY, **{k: None for k, _ in table if k != "tb_count"})
    with pytest.raises(TypeError, match="'solve_depth0'"):
        nat.selfplay_args(ENTRY, **{k: None for k, _ in table}, solve_depth0=0)


def _collect(world, start, n, policies, search, **kw):
    env = positions_env(world, start, n)
    env._lib = Counting(env._lib)
    return env.collect(4, policies=policies, search=search, out="fresh", **kw), env


def test_collect_surface(cpu, world, start, nets):
    net = nets[64]
    ev = _evaluator(net)
    big = python_table(world)
    base = dict(evaluator=ev, iterations=(8, 12), sample_plies=2, explore=24)
    # which entry point each spelling reaches
    for policies, gumbel, entry, judged in (
            (("evaluator", "tablebase"), dict(considered=16, tablebase=big), ENTRY, False),
            (("evaluator", "tablebase"), dict(considered=16, tablebase=big, judge=True), ENTRY, True),
            (("evaluator", "evaluator"), dict(considered=(16, 0), tablebase=big, judge=True, tb_mode="shortest", tb_count=600), ENTRY, True),
            (("evaluator", "evaluator"), dict(considered=0, tablebase=big, judge=True), ENTRY, True),
            (("evaluator", "evaluator"), dict(considered=16, tablebase=big), ENTRY, False),  # (nobody reads the table: the parent's launch)
            (("tablebase", "random"), dict(tablebase=big, judge=True), ENTRY, True),
            (("tablebase", G.TablebaseGobbletPolicy(big)), dict(judge=True), ENTRY, True),  # (a policy instance supplies its table)
            (("evaluator", "evaluator"), dict(considered=16), "gbl_collect_search_gumbel", False),
            (("evaluator", "evaluator"), dict(considered=16, solve_depth=2), "gbl_collect_gumbel_solve", False)):
        tr, env = _collect(world, start, 65, policies, dict(base, gumbel=gumbel))
        assert set(env._lib.calls) == {entry}, (gumbel, env._lib.calls)
        assert all((k in tr) == judged for k in ("tb_outcomes", "tb_value", "tb_played")), gumbel
        assert ("outcomes" in tr) == (entry == "gbl_collect_gumbel_solve")
    tr, env = _collect(world, start, 65, ("evaluator", "tablebase"), dict(evaluator=ev, iterations=4, tablebase=big, judge=True))  # as before
    assert set(env._lib.calls) == {"gbl_collect_search_tb"} and "outcomes" not in tr
    # the new keys, and the window against the raw entry point
    got, env = _collect(world, start, 65, ("evaluator", "tablebase"),
                        dict(base, gumbel=dict(considered=(5, 99), scale=40, noise=True, tablebase=big, tb_mode="shortest", tb_count=7, judge=True)))
    assert got["tb_outcomes"].shape == (4, 65, 54) and got["tb_outcomes"].dtype == torch.int8
    assert got["tb_value"].shape == got["tb_played"].shape == (4, 65) and got["tb_played"].dtype == torch.int8
    st, tm, turn = (x[:65] for x in start)
    raw = host_collect_gtb(world[1], st, tm, turn, 4, ("eval", "tb"), (net, None), (8, 0), (5, 0), 1, 50, 40, 24, 2, nat.ILLEGAL_NOOP, "time", 11, 3,
                           0, mode=1, count=7)[0]
    for k in raw:
        assert np.array_equal(got[k].numpy().reshape(raw[k].shape), raw[k]), k
    how = got["how"].numpy()
    assert {nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED, nat.HOW_GUMBEL, nat.HOW_RANDOM} <= set(np.unique(how).tolist())
    tile, _ = _collect(world, start, 65, ("evaluator", "tablebase"), dict(base, gumbel=dict(tablebase=big, judge=True)), layout="tile")
    assert tile["tb_outcomes"].shape == (2, 4, 64, 54)
    # every new ValueError
    half = G.Tablebase((1, 1, 0), "cpu")
    half.build(max_sweeps=1)
    assert not half.complete
    _collect(world, start, 8, ("evaluator", "tablebase"), dict(base, gumbel=dict(tablebase=half, allow_incomplete=True)))
    for bad in (dict(tablebase=big, solve_depth=2), dict(judge=True, tablebase=big, solve_depth=(0, 1)), dict(tablebase=half),
                dict(tablebase=big, tb_mode="best"), dict(tablebase=big, tb_count=0), dict(tablebase=big, tb_count=601), dict(judge=True),
                dict(tablebase=None, judge=True), dict(tablebase=big, bogus=1), dict(tablebase=big, considered=55),
                dict(tablebase=big, scale=65), dict(tb_mode="result"), dict(tablebase="tb")):
        with pytest.raises(ValueError):
            _collect(world, start, 8, ("evaluator", "evaluator"), dict(base, gumbel=bad))
    with pytest.raises(ValueError, match="lives on"):  # the table on another device
        other = G.Tablebase.__new__(G.Tablebase)
        other.__dict__.update(big.__dict__)
        other.device = torch.device("cuda:0")
        _collect(world, start, 8, ("evaluator", "tablebase"), dict(base, gumbel=dict(tablebase=other)))
    for beside in (dict(tablebase=big), dict(judge=True), dict(tb_count=3), dict(solve_depth=2), dict(noise=0.25),
                   dict(cap=dict(fast_iterations=2, full=0.25))):  # beside gumbel=: refused
        with pytest.raises(ValueError, match="gumbel"):
            _collect(world, start, 8, ("evaluator", "evaluator"), dict(base, gumbel=dict(tablebase=big, judge=True), **beside))
    with pytest.raises(ValueError, match="gumbel"):  # as before: the table beside a gumbel dict without it
        _collect(world, start, 8, ("tablebase", "evaluator"), dict(base, tablebase=big, gumbel=dict(considered=16)))
    with pytest.raises(ValueError):
        _collect(world, start, 8, ("tablebase", "greedy"), dict(gumbel=dict(tablebase=big)))
    # the single decision and reanalysis: the table's keys stay unknown there, and the message names the policy that composes it
    with pytest.raises(ValueError, match="TablebaseGobbletPolicy"):
        G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=16, gumbel=dict(tablebase=big), device="cpu")
    from gobblet_rl_amd.evaluator_policy import gumbel_args
    for key in ("tablebase", "tb_mode", "tb_count", "judge", "allow_incomplete"):
        with pytest.raises(ValueError, match=r"TablebaseGobbletPolicy\(tb, fallback="):
            gumbel_args({"considered": 16, key: 1})
