"""Playout-cap randomisation on the MI355X (-m gpu): gbl_collect_search_cap against the host flavour, bit for bit and between canaries;
shares (256, 256) against gbl_collect_search_noise on the device; and one graph capture and replay of collect(..., cap=) with the ply
on the device.  The shapes are the smallest at which the kernel can still go wrong: a single board, a ragged second tile and a ragged
third; budgets (8, 3) and (12, 1), so that the tree of the previous ply is larger than this ply's budget (a stale node read would
show); board 0 at seed 7 plays a full ply after a fast one; and the budget differs between neighbouring wavefronts.  Depth 3 takes the
solver's LDS path and its fence beside a budget that changes between plies."""
import numpy as np
import pytest
import torch

from tests import cap_restatement as CR
from tests import evaluator_restatement as R
from tests import selfplay_harness as H
from tests.search_harness import DEV, G  # noqa: F401  (G: the fixture)
from tests.selfplay_cap_harness import FULL, device_collect_cap, host_collect_cap
from tests.selfplay_harness import DeviceNet, _evaluator, same
from tests.test_selfplay_solve import EXPLORE, fixture_boards, smoke_net

pytestmark = pytest.mark.gpu

SEED, T = 7, 6


@pytest.fixture(scope="module")
def boards(G):
    """Boards 0 .. 39 empty (board 0 plays the pinned draws of seed 7 from ply 0), then the midgame fixture."""
    st, tm, turn = fixture_boards(90, DEV)
    return (np.ascontiguousarray(np.concatenate([np.zeros((40, 27), np.int8), st])), np.concatenate([np.zeros(40, np.int8), tm]),
            np.concatenate([np.zeros(40, np.int32), turn % 6]).astype(np.int32))


@pytest.fixture(scope="module")
def nets(G):
    """(host nets, device nets): H = 64 against 128."""
    pair = (smoke_net(), R.random_net(128, 77))
    return pair, tuple(DeviceNet(x) for x in pair)


@pytest.mark.parametrize("depth", [0, 3])
@pytest.mark.parametrize("n", [1, 65, 130])
def test_k_collect_cap_equals_host_flavour(G, boards, nets, n, depth):
    hn, dn = nets
    st, tm, turn = (x[:n] for x in boards)
    seen = set()
    for (its, fast), layout in ((((8, 8), (3, 3)), "time"), (((12, 12), (1, 1)), "tile")):
        for share in ((128, 64), (0, FULL), (FULL, 0)):
            kw = dict(deps=(depth, depth), noise=(64, 0), X=EXPLORE, sample_plies=4, layout=layout, seed=SEED)
            got = device_collect_cap(st, tm, turn, T, ("eval", "eval"), dn, its, fast, share, **kw)
            same(got, host_collect_cap(st, tm, turn, T, ("eval", "eval"), hn, its, fast, share, **kw))
            how = got[0]["how"]
            seen |= set(np.unique(how).tolist())
            if share == (128, 64) and depth == 0:  # board 0, seed 7: full at plies 1 and 3 -- a full ply after a fast one
                assert [int(h) <= 4 for h in how[:, 0]] == [CR.is_full(SEED, 0, q, share[q & 1]) for q in range(T)]
                assert [CR.is_full(SEED, 0, q, 128) for q in range(T)] == [False, True, False, True, False, False]
                if n > 1:  # the budget differs between neighbouring wavefronts
                    assert ((how[:, :-1] <= 4) != (how[:, 1:] <= 4)).any()
    nat = G._native
    assert {nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED, nat.HOW_FAST, nat.HOW_FAST_SAMPLED} <= seen
    assert depth == 0 or n == 1 or nat.HOW_PROVEN in seen


def test_full_shares_are_the_noise_launch(G, boards, nets):
    """Shares (256, 256) through the new entry point against gbl_collect_search_noise, both on the device; and a RANDOM side, whose
    parameters are not read, with the ply index through ply_dev."""
    hn, dn = nets
    st, tm, turn = (x[:65] for x in boards)
    got = device_collect_cap(st, tm, turn, T, ("eval", "eval"), dn, (8, 3), (-1, 99), (FULL, FULL), (3, 0), (64, 0), EXPLORE, 4, seed=SEED,
                             env_base=(1 << 40) + 3, ply0=4)
    exp = H.device_collect("noise", st, tm, turn, T, ("eval", "eval"), EXPLORE, 4, 0, "time", SEED, (1 << 40) + 3, 4, nets=dn, its=(8, 3),
                           deps=(3, 0), noise=(64, 0))
    same(got, exp)
    kw = dict(deps=(9, 2), noise=(999, 128), X=16, sample_plies=2, seed=1, ply0=0, ply_dev=7)
    same(device_collect_cap(st, tm, turn, T, ("random", "eval"), (None, dn[1]), (0, 8), (77, 2), (-4, 100), **kw),
         host_collect_cap(st, tm, turn, T, ("random", "eval"), (None, hn[1]), (0, 8), (0, 2), (FULL, 100), **kw))


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "outcomes", "proven", "observation", "done")


def test_graph_capture_and_replay(G):
    """One captured capped launch with ply_dev, replayed twice (gbl_counter_add advances the ply inside the graph): the two replays
    differ and each equals the HOST flavour's window at the advanced ply, so the cap's draw moves with *ply_dev."""
    n, T_, seed = 130, 3, 7
    net = smoke_net()
    kw = lambda d: dict(policies=("evaluator", "evaluator"),  # noqa: E731
                        search=dict(evaluator=_evaluator(net, d), iterations=8, solve_depth=(2, 0), sample_plies=2, noise=(0.25, 1.0),
                                    cap=dict(fast_iterations=(3, 1), full=(0.5, 0.25))))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    env.rollout(20)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T_, search_outputs=True, evaluator_outputs=True, solver_outputs=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    seen = []
    kd = kw(DEV)
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            env.collect(T_, out=buf, **kd)
            env.advance_ply()
        for i in range(2):
            g.replay()
            side.synchronize()
            seen.append({k: buf[k].clone() for k in KEYS})
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = G.BatchedGobblet(n, "cpu", auto_reset=True, seed=seed, track_turn=True)
    ref.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})
    kc = kw("cpu")
    for i in range(2):
        out = ref.collect(T_, out="fresh", **kc)
        for k in KEYS:
            assert torch.equal(out[k], seen[i][k].cpu()), (i, k)
        assert (out["how"] >= G._native.HOW_FAST).any() and (out["how"] <= G._native.HOW_SEARCH_SAMPLED).any()
    assert torch.equal(env.squares.cpu(), ref.squares) and torch.equal(env.turn.cpu(), ref.turn)
    assert not torch.equal(seen[0]["how"], seen[1]["how"]) and not torch.equal(seen[0]["actions"], seen[1]["actions"])
