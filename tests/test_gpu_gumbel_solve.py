"""gbl_collect_gumbel_solve on the MI355X (-m gpu): k_collect_gumbel_solve against the host flavour, bit for bit and with canaries of
16 elements around every output, at n = 1 / 65 / 130 on the four cases of tests/gumbel_solve_harness.py in both layouts and with both
networks; the guard's two arrays at odd addresses; the two identities on the device (depths 0: gbl_collect_search_gumbel, considered 0:
gbl_collect_search_solve); and one graph capture with ply_dev, replayed twice."""
import numpy as np
import pytest
import torch

from tests import evaluator_restatement as R
from tests import solver_restatement as SR
from tests import selfplay_harness as H
from tests.gumbel_harness import device_collect_gumbel
from tests.gumbel_solve_harness import CASES, CENSUS, EXPLORE, census, device_collect_gs, host_collect_gs
from tests.search_harness import G  # noqa: F401  (the fixture)
from tests.selfplay_harness import DEV, DeviceNet, _evaluator, same
from tests.test_selfplay_solve import fixture_boards, smoke_net

pytestmark = pytest.mark.gpu

SEED, ENV_BASE, PLY0, T = 0xFEDCBA9876543210, (1 << 41) + 77, 3, 6


@pytest.fixture(scope="module")
def c5(G):
    st, tm, turn = fixture_boards(130)
    return st, tm, turn % 5


@pytest.fixture(scope="module")
def nets(G):
    """{hidden: (host net, device net)}: smoke()'s network and a second one of another width."""
    return {x.w1.shape[1]: (x, DeviceNet(x)) for x in (smoke_net(), R.random_net(128, 77))}


# (layout, sample_plies, gumbel_noise, scale, hidden, illegal_mode) of a case's two runs
RUNS = {0: (("time", 0, 1, 23, 64, 0), ("tile", 0, 0, 0, 128, 1)), 1: (("time", 2, 1, 23, 128, 1), ("tile", 0, 1, 0, 64, 0)),
        2: (("time", 0, 1, 0, 128, 0), ("tile", 0, 0, 23, 64, 1)), 3: (("time", 0, 1, 23, 64, 1), ("tile", 0, 1, 0, 128, 0))}


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("n", [1, 65, 130])
def test_device_equals_host_flavour(G, c5, nets, n, case):
    pols, considered, deps, its = CASES[case]
    st, tm, turn = c5[0][:n], c5[1][:n], c5[2][:n]
    for layout, sample_plies, noise, scale, hidden, illegal_mode in RUNS[case]:
        hn, dn = nets[hidden]
        args = (its, deps, considered, noise, 50, scale, EXPLORE, sample_plies, illegal_mode, layout, SEED, ENV_BASE)
        got = device_collect_gs(st, tm, turn, T, pols, tuple(dn if p == "eval" else None for p in pols), *args, PLY0 - 2, ply_dev=2)
        same(got, host_collect_gs(st, tm, turn, T, pols, tuple(hn if p == "eval" else None for p in pols), *args, PLY0))
    if n >= 65:  # every branch of the fixture's first ply, by the solver alone, and the codes they leave
        for depth in {d for d in deps if d}:
            assert tuple(int(x) for x in census(st, tm, depth)[0]) == CENSUS[(n, depth)]
        how = got[0]["how"]
        assert (how == G._native.HOW_PROVEN).any() and (how == G._native.HOW_GUMBEL).any()
        assert (got[0]["proven"] > 0).any() and (got[0]["proven"] < 0).any()


def test_the_guards_arrays_at_odd_addresses(G, c5, nets):
    hn, dn = nets[64]
    pols, considered, deps, its = CASES[0]
    for layout in ("time", "tile"):
        args = (its, deps, considered, 1, 50, 23, EXPLORE, 0, 0, layout, SEED, ENV_BASE, PLY0)
        got = device_collect_gs(*c5, T, pols, (dn, dn), *args, odd=("outcomes", "proven"))
        same(got, host_collect_gs(*c5, T, pols, (hn, hn), *args))
    keep = ("actions", "outcomes", "proven")  # ... and with most of the others NULL
    got = device_collect_gs(*c5, T, pols, (dn, dn), *args, odd=("outcomes", "proven"), keep=keep)
    assert set(got[0]) == set(keep)
    same(got, host_collect_gs(*c5, T, pols, (hn, hn), *args, keep=keep))


def test_identities_on_the_device(G, c5, nets):
    st, tm, turn = c5
    dn = (nets[64][1], nets[128][1])
    for layout in ("time", "tile"):
        # both depths 0: every shared array is gbl_collect_search_gumbel's -- with the guard's two arrays (this entry point's kernel
        # fills them) and without them (gbl_collect_search_gumbel's own kernel runs)
        exp = device_collect_gumbel(st, tm, turn, T, ("eval", "eval"), dn, (8, 16), (16, 0), 1, 50, 23, EXPLORE, 3, 0, layout, SEED, ENV_BASE, PLY0)
        got = device_collect_gs(st, tm, turn, T, ("eval", "eval"), dn, (8, 16), (0, 0), (16, 0), 1, 50, 23, EXPLORE, 3, 0, layout, SEED, ENV_BASE, PLY0)
        assert (got[0].pop("outcomes") == SR.NONE).all() and (got[0].pop("proven") == 0).all()
        same(got, exp)
        same(device_collect_gs(st, tm, turn, T, ("eval", "eval"), dn, (8, 16), (0, 0), (16, 0), 1, 50, 23, EXPLORE, 3, 0, layout, SEED, ENV_BASE,
                               PLY0, keep=list(exp[0])), exp)
        # both considered 0: every array is gbl_collect_search_solve's, whatever the rule's three say
        got = device_collect_gs(st, tm, turn, T, ("eval", "eval"), dn, (8, 16), (2, 3), (0, 0), 5, -3, 999, EXPLORE, 3, 1, layout, SEED, ENV_BASE, PLY0)
        same(got, H.device_collect("solve", st, tm, turn, T, ("eval", "eval"), EXPLORE, 3, 1, layout, SEED, ENV_BASE, PLY0, nets=dn, its=(8, 16),
                                   deps=(2, 3)))


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "outcomes", "proven", "observation", "done")


def test_graph_capture_and_replay(G):
    """One captured guarded Gumbel launch with ply_dev, replayed twice (gbl_counter_add advances the ply inside the graph): the same
    as two eager launches."""
    n, T_, seed = 300, 3, 7
    ev = _evaluator(smoke_net(), DEV)
    kw = dict(policies=("evaluator", "evaluator"), search=dict(evaluator=ev, iterations=16, gumbel=dict(considered=(16, 4), solve_depth=(2, 3))))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    env.rollout(20)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T_, search_outputs=True, evaluator_outputs=True, solver_outputs=True)
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
    assert (how == G._native.HOW_PROVEN).any() and (how == G._native.HOW_GUMBEL).any() and not torch.equal(seen[0]["actions"], seen[1]["actions"])
    # ... and the same window on the host flavour
    cpu = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, track_turn=True)
    cpu.rollout(20)
    out = cpu.collect(T_, out="fresh", policies=kw["policies"], search=dict(kw["search"], evaluator=ev.to("cpu")))
    for k in KEYS:
        assert np.array_equal(out[k].numpy(), seen[0][k].cpu().numpy()), k
