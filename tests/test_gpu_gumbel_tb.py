"""gbl_collect_gumbel_tb on the MI355X (-m gpu): k_collect_gumbel_tb against the host flavour, bit for bit and with canaries of 16
elements around every output, at n = 1 / 65 / 130 on the six cases of tests/gumbel_tb_harness.py in both layouts and with both
networks; the judge arrays at odd addresses and aux at a shifted one; the two identities on the device with and without judge arrays,
so that every dispatch of the entry point is hit (its own kernel, gbl_collect_search_gumbel's, gbl_collect_search_tb's); the
search-free dispatch against gbl_collect_search_tb on the device; and one graph capture with ply_dev, replayed twice."""
import numpy as np
import pytest
import torch

from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests import selfplay_tb_harness as TBH
from tests import tablebase_harness as TH
from tests.gumbel_harness import device_collect_gumbel
from tests.gumbel_tb_harness import CASES, EXPLORE, INVENTORY, JUDGE, SHARED, boards, device_collect_gtb, host_collect_gtb, judge_keep
from tests.search_harness import G  # noqa: F401  (the fixture)
from tests.selfplay_harness import DEV, DeviceNet, _evaluator, same
from tests.test_selfplay_solve import smoke_net

pytestmark = pytest.mark.gpu

SEED, ENV_BASE, PLY0, T = 0xFEDCBA9876543210, (1 << 41) + 77, 3, 6


@pytest.fixture(scope="module")
def world(G):
    """The (2, 2, 0) table built on the device and copied to the host: (device Table, host Table, host flavour, G.Tablebase)."""
    tb = G.Tablebase(INVENTORY, DEV)
    tb.build()
    assert tb.complete
    host = TH.Host(INVENTORY)
    assert np.array_equal(tb._aux.cpu().numpy(), host.aux)
    return TBH.Table(INVENTORY, tb._aux, tb.table), TBH.Table(INVENTORY, host.aux, tb.table.cpu().numpy()), host, tb


@pytest.fixture(scope="module")
def start(world):
    return boards(world[2], 130)


@pytest.fixture(scope="module")
def nets(G):
    """{hidden: (host net, device net)}: smoke()'s network and a second one of another width."""
    return {x.w1.shape[1]: (x, DeviceNet(x)) for x in (smoke_net(), R.random_net(128, 77))}


# (layout, sample_plies, gumbel_noise, scale, hidden, illegal_mode, tb_mode, tb_count) of a case's two runs
RUNS = {0: (("time", 0, 1, 23, 64, 0, 0, 1), ("tile", 2, 0, 0, 128, 1, 1, 7)), 1: (("time", 0, 1, 23, 128, 0, 0, 1), ("tile", 2, 0, 0, 64, 1, 1, 7)),
        2: (("time", 2, 1, 23, 64, 0, 0, 1), ("tile", 0, 0, 0, 128, 1, 1, 7)), 3: (("time", 0, 1, 23, 128, 0, 0, 1), ("tile", 0, 0, 0, 64, 1, 1, 7)),
        4: (("time", 0, 1, 23, 64, 0, 0, 1), ("tile", 2, 0, 0, 64, 1, 1, 600)), 5: (("time", 0, 1, 23, 64, 0, 0, 1), ("tile", 2, 0, 0, 64, 1, 1, 7))}


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("n", [1, 65, 130])
def test_device_equals_host_flavour(G, world, start, nets, n, case):
    dev, hst, _, _ = world
    pols, considered, its, judge = CASES[case]
    st, tm, turn = (x[:n] for x in start)
    hows = set()
    for layout, sample_plies, noise, scale, hidden, illegal_mode, mode, count in RUNS[case]:
        hn, dn = nets[hidden]
        args = (its, considered, noise, 50, scale, EXPLORE, sample_plies, illegal_mode, layout, SEED, ENV_BASE)
        kw = dict(mode=mode, count=count, keep=judge_keep(judge))
        got = device_collect_gtb(dev, st, tm, turn, T, pols, tuple(dn if p == "eval" else None for p in pols), *args, PLY0 - 2, ply_dev=2, **kw)
        same(got, host_collect_gtb(hst, st, tm, turn, T, pols, tuple(hn if p == "eval" else None for p in pols), *args, PLY0, **kw))
        hows |= set(got[0]["how"].ravel().tolist())
    if n >= 65:  # the codes the case's branches leave
        if "tb" in pols:
            assert {nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED, nat.HOW_RANDOM} <= hows
        if any(considered):
            assert nat.HOW_GUMBEL in hows
        if judge:
            empty = (got[0]["tb_outcomes"] == nat.SOLVE_NONE).all(-1)
            assert empty.any() and not empty.all()


def test_judge_arrays_at_odd_addresses_and_aux_shifted(G, world, start, nets):
    dev, hst, _, _ = world
    hn, dn = nets[64]
    shifted = torch.zeros(nat.TB_AUX_BYTES + 16, dtype=torch.uint8, device=DEV)  # aux + 16: another 16-byte aligned address
    shifted[16:].copy_(dev.aux)
    moved = TBH.Table(INVENTORY, shifted[16:], dev.table)
    assert moved.aux.data_ptr() % 16 == 0 and moved.aux.data_ptr() != dev.aux.data_ptr()
    pols, considered, its, judge = CASES[0]
    for layout in ("time", "tile"):
        args = (its, considered, 1, 50, 23, EXPLORE, 2, 0, layout, SEED, ENV_BASE, PLY0)
        got = device_collect_gtb(moved, *start, T, pols, (dn, None), *args, mode=1, count=5, odd=JUDGE)
        same(got, host_collect_gtb(hst, *start, T, pols, (hn, None), *args, mode=1, count=5))
    keep = ("actions",) + JUDGE  # ... and with most of the others NULL
    got = device_collect_gtb(moved, *start, T, pols, (dn, None), *args, mode=1, count=5, odd=JUDGE, keep=keep)
    assert set(got[0]) == set(keep)
    same(got, host_collect_gtb(hst, *start, T, pols, (hn, None), *args, mode=1, count=5, keep=keep))
    for one in JUDGE:  # each judge array alone makes every ply probed
        keep = ("actions", one)
        same(device_collect_gtb(dev, *start, T, ("eval", "eval"), (dn, dn), (8, 8), (16, 4), keep=keep, seed=SEED),
             host_collect_gtb(hst, *start, T, ("eval", "eval"), (hn, hn), (8, 8), (16, 4), keep=keep, seed=SEED))


def test_identities_on_the_device(G, world, start, nets):
    dev, hst, _, _ = world
    st, tm, turn = start
    dn = (nets[64][1], nets[128][1])
    for layout in ("time", "tile"):
        # no TABLEBASE side: with the judge arrays NULL gbl_collect_search_gumbel's own kernel runs (the table may be NULL); with them
        # this entry point's kernel does, and every shared array is still gbl_collect_search_gumbel's
        exp = device_collect_gumbel(st, tm, turn, T, ("eval", "eval"), dn, (8, 16), (16, 0), 1, 50, 23, EXPLORE, 3, 0, layout, SEED, ENV_BASE, PLY0)
        for table in (None, dev):
            same(device_collect_gtb(table, st, tm, turn, T, ("eval", "eval"), dn, (8, 16), (16, 0), 1, 50, 23, EXPLORE, 3, 0, layout, SEED, ENV_BASE,
                                    PLY0, keep=list(SHARED)), exp)
        got = device_collect_gtb(dev, st, tm, turn, T, ("eval", "eval"), dn, (8, 16), (16, 0), 1, 50, 23, EXPLORE, 3, 0, layout, SEED, ENV_BASE, PLY0)
        for k in JUDGE:
            got[0].pop(k)
        same(got, exp)
        # both considered 0: every shared array is gbl_collect_search_tb's at depths (0, 0) and noise (0, 0), whatever the rule's three
        # say -- with and without judge arrays, a table side or not
        for pols, use, its in ((("eval", "tb"), (dn[0], None), (8, 0)), (("eval", "eval"), dn, (8, 16))):
            for judge in (True, False):
                keep = judge_keep(judge)
                got = device_collect_gtb(dev, st, tm, turn, T, pols, use, its, (0, 0), 5, -3, 999, EXPLORE, 3, 1, layout, SEED, ENV_BASE, PLY0,
                                         mode=1, count=9, keep=keep)
                exp_tb = TBH.device_collect_tb(dev, st, tm, turn, T, pols, use, its, (0, 0), (0, 0), EXPLORE, 3, 1, layout, SEED, ENV_BASE, PLY0,
                                               None, 1, 9, keep)
                exp_tb[0].pop("outcomes", None), exp_tb[0].pop("proven", None)
                same(got, exp_tb)


def test_the_search_free_dispatch(G, world, start):
    """(TB, TB) and (TB, RANDOM): no EVAL_TREE side, so gbl_collect_search_tb's search-free instantiation runs, whatever the rule's
    arguments say; against gbl_collect_search_tb on the device and the host flavour of this entry point."""
    dev, hst, _, _ = world
    st, tm, turn = start
    for pols in (("tb", "tb"), ("tb", "random"), ("random", "tb")):
        for layout, sample_plies, mode, count in (("time", 0, 0, 1), ("tile", 2, 1, 600)):
            got = device_collect_gtb(dev, st, tm, turn, T, pols, (None, None), (0, 0), (16, 54), 1, 50, 23, EXPLORE, sample_plies, 1, layout, SEED,
                                     ENV_BASE, PLY0, mode=mode, count=count)
            same(got, host_collect_gtb(hst, st, tm, turn, T, pols, (None, None), (0, 0), (16, 54), 1, 50, 23, EXPLORE, sample_plies, 1, layout, SEED,
                                       ENV_BASE, PLY0, mode=mode, count=count))
            exp = TBH.device_collect_tb(dev, st, tm, turn, T, pols, (None, None), (0, 0), (0, 0), (0, 0), EXPLORE, sample_plies, 1, layout, SEED,
                                        ENV_BASE, PLY0, None, mode, count)
            assert (exp[0].pop("outcomes") == nat.SOLVE_NONE).all() and (exp[0].pop("proven") == 0).all()
            same(got, exp)
            assert not got[0]["nodes"].any() and not got[0]["priors"].any()


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "tb_outcomes", "tb_value", "tb_played", "observation",
        "done")


def test_graph_capture_and_replay(G, world):
    """One captured Gumbel-against-table launch with ply_dev and the judge on, replayed twice (gbl_counter_add advances the ply inside
    the graph): the same as two eager launches."""
    n, T_, seed = 300, 3, 7
    tb = world[3]
    ev = _evaluator(smoke_net(), DEV)
    kw = dict(policies=("tablebase", "evaluator"),
              search=dict(evaluator=ev, iterations=16, sample_plies=2, gumbel=dict(considered=16, tablebase=tb, tb_count=3, judge=True)))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T_, search_outputs=True, evaluator_outputs=True, tablebase_outputs=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    seen = []
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            env.collect(T_, out=buf, **kw)
            env.advance_ply()
        for i in range(2):
            g.replay()
            side.synchronize()
            seen.append({k: buf[k].clone() for k in KEYS})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    ref.load_state_dict(sd)
    for i in range(2):
        out = ref.collect(T_, out="fresh", **kw)
        for k in KEYS:
            assert torch.equal(out[k], seen[i][k]), (i, k)
    assert torch.equal(env.squares, ref.squares) and torch.equal(env.turn, ref.turn)
    how = seen[0]["how"]
    assert (how == nat.HOW_TABLE_SAMPLED).any() and (how == nat.HOW_GUMBEL).any()  # (fresh boards: the table's plies lie inside sample_plies)
    assert not torch.equal(seen[0]["actions"], seen[1]["actions"])
    # ... and the same window on the host flavour, Tablebase.judge included
    cpu_tb = G.Tablebase(INVENTORY, "cpu")
    cpu_tb.table.copy_(tb.table.cpu())
    cpu_tb.sweeps, cpu_tb.complete = tb.sweeps, True
    cpu = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, track_turn=True)
    search = dict(kw["search"], evaluator=ev.to("cpu"), gumbel=dict(kw["search"]["gumbel"], tablebase=cpu_tb))
    out = cpu.collect(T_, out="fresh", policies=kw["policies"], search=search)
    for k in KEYS:
        assert np.array_equal(out[k].numpy(), seen[0][k].cpu().numpy()), k
    first = {k: v for k, v in seen[0].items()}
    assert tb.judge(first) == cpu_tb.judge(out)
