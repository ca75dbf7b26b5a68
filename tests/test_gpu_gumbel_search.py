"""The Gumbel root search on the MI355X (-m gpu): gbl_tree_search_gumbel and gbl_collect_search_gumbel against the host flavour, byte
for byte and between canaries (the host flavour is pinned to the restatement of the header's text in tests/test_gumbel_search.py);
(0, 0) against gbl_collect_search_eval on the device; and one graph capture and replay of collect(..., gumbel=) with the ply on the
device.  The shapes are the smallest at which the kernel can still go wrong: a single board, a ragged second tile and a ragged third;
roots of 54, 27, 2, 1 and 0 candidates under a mask; every schedule of tests/gumbel_harness.py::PAIRS but the long one (that one, and
the longer ones of LONG_PAIRS, in tests/test_gpu_gumbel_long.py) -- a considered
set of one, of two (never halved), of three and five (odd halvings), of sixteen at one visit each, and of more than the candidates."""
import numpy as np
import pytest
import torch

from tests import evaluator_restatement as R
from tests import selfplay_harness as H
from tests.gumbel_harness import GUMBEL_NAMES, PAIRS, device_collect_gumbel, host_collect_gumbel, rule_boards
from tests.search_harness import DEV, G, run  # noqa: F401  (G: the fixture)
from tests.search_harness import same as same_arrays
from tests.selfplay_harness import DeviceNet, _evaluator, same
from tests.test_selfplay_solve import EXPLORE, fixture_boards, smoke_net

pytestmark = pytest.mark.gpu

SEED, ENV_BASE, T = 0xFEDCBA9876543210, (1 << 41) + 77, 6


@pytest.fixture(scope="module")
def roots(G):
    """130 roots: the last eight under masks of 27, 2, 1 and 0 candidates.  n = 1 / 65 are the LAST boards, so every size has them."""
    st, tm, _ = fixture_boards(120, DEV)
    return rule_boards((st, tm))[:3]


@pytest.fixture(scope="module")
def boards(G):
    """Boards 0 .. 39 empty, then the midgame fixture."""
    st, tm, turn = fixture_boards(90, DEV)
    return (np.ascontiguousarray(np.concatenate([np.zeros((40, 27), np.int8), st])), np.concatenate([np.zeros(40, np.int8), tm]),
            np.concatenate([np.zeros(40, np.int32), turn % 6]).astype(np.int32))


@pytest.fixture(scope="module")
def nets(G):
    """(host nets, device nets): H = 64 against 128."""
    pair = (smoke_net(), R.random_net(128, 77))
    return pair, tuple(DeviceNet(x) for x in pair)


@pytest.mark.parametrize("pair", [p for p in PAIRS if p != (16, 64)])
@pytest.mark.parametrize("n", [1, 65, 130])
def test_k_tree_gumbel_equals_host_flavour(G, roots, nets, n, pair):
    hn, dn = nets
    st, tm, mask = (x[-n:] for x in roots)
    considered, iterations = pair
    for noise in (0, 1):
        for scale in (0, 23):
            k = noise ^ (scale != 0)  # H = 64 and 128, either against every noise and scale over the pairs
            params = (iterations, EXPLORE, considered, noise, 50, scale, SEED, ENV_BASE, 5)
            got = run("tree_search_gumbel", DEV, st, tm, mask, params, dn[k])
            same_arrays(got, run("tree_search_gumbel", "cpu", st, tm, mask, params, hn[k]))
            assert (got["gumbel"] != 0).any() == bool(noise and mask.any()) and (got["target"].max(1) > 0).sum() == (mask.any(1)).sum()
    # every output is optional, and the least aligned addresses serve
    same_arrays(run("tree_search_gumbel", DEV, st, tm, mask, params, dn[k], keep=("action", "target"), misaligned=True),
                {x: got[x] for x in ("action", "target")})
    assert tuple(got) == GUMBEL_NAMES


@pytest.mark.parametrize("n", [1, 65, 130])
def test_k_collect_gumbel_equals_host_flavour(G, boards, nets, n):
    hn, dn = nets
    st, tm, turn = (x[:n] for x in boards)
    seen = set()
    for considered, pols in (((16, 0), ("eval", "eval")), ((0, 4), ("eval", "eval")), ((3, 54), ("eval", "eval")), ((16, 9), ("eval", "random"))):
        for layout, noise, scale in (("time", 1, 23), ("tile", 0, 46)):
            kw = dict(noise=noise, scale=scale, X=EXPLORE, sample_plies=4, layout=layout, seed=SEED, env_base=ENV_BASE, ply0=3)
            d_nets, h_nets = ((dn[0], None), (hn[0], None)) if pols[1] == "random" else (dn, hn)
            got = device_collect_gumbel(st, tm, turn, T, pols, d_nets, (8, 16), considered, **kw)
            same(got, host_collect_gumbel(st, tm, turn, T, pols, h_nets, (8, 16), considered, **kw))
            how, mover = got[0]["how"], got[0]["mover"]
            seen |= set(np.unique(how).tolist())
            for m in range(2):  # a Gumbel side's plies are all GBL_HOW_GUMBEL, and its rows are target bytes
                rule = pols[m] == "eval" and considered[m] > 0
                assert ((how[mover == m] == G._native.HOW_GUMBEL) == rule).all()
                if rule:
                    rows = got[0]["visits"][mover == m]
                    assert rows.max() <= 255 and (rows.sum(1) >= 255).all()
    nat = G._native
    assert {nat.HOW_GUMBEL, nat.HOW_SEARCH, nat.HOW_SEARCH_SAMPLED} <= seen and (n == 1 or nat.HOW_RANDOM in seen)


def test_no_gumbel_side_is_the_eval_launch(G, boards, nets):
    """(0, 0) through the new entry point against gbl_collect_search_eval, both on the device (the rule's three are then not read), and
    with the ply index through ply_dev."""
    hn, dn = nets
    st, tm, turn = (x[:65] for x in boards)
    got = device_collect_gumbel(st, tm, turn, T, ("eval", "eval"), dn, (8, 3), (0, 0), noise=7, visit_offset=-1, scale=999, X=EXPLORE,
                                sample_plies=4, seed=SEED, env_base=(1 << 40) + 3, ply0=4)
    same(got, H.device_collect("eval", st, tm, turn, T, ("eval", "eval"), EXPLORE, 4, 0, "time", SEED, (1 << 40) + 3, 4, nets=dn, its=(8, 3)))
    kw = dict(X=16, sample_plies=2, seed=1, ply0=0, ply_dev=7)
    same(device_collect_gumbel(st, tm, turn, T, ("random", "eval"), (None, dn[1]), (0, 8), (99, 5), **kw),
         host_collect_gumbel(st, tm, turn, T, ("random", "eval"), (None, hn[1]), (0, 8), (0, 5), **kw))


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "root_value", "priors", "observation", "done")


def test_graph_capture_and_replay(G):
    """One captured Gumbel launch with ply_dev, replayed twice (gbl_counter_add advances the ply inside the graph): the two replays
    differ and each equals the HOST flavour's window at the advanced ply, so the Gumbel row moves with *ply_dev."""
    n, T_, seed = 130, 3, 7
    net = smoke_net()
    kw = lambda d: dict(policies=("evaluator", "evaluator"),  # noqa: E731
                        search=dict(evaluator=_evaluator(net, d), iterations=8, gumbel=dict(considered=(4, 16))))
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=seed, track_turn=True)
    env.rollout(20)
    env.device_ply()
    sd = env.state_dict()
    buf = env.trajectory_buffers(T_, search_outputs=True, evaluator_outputs=True)
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
        assert (out["how"] == G._native.HOW_GUMBEL).all()
    assert torch.equal(env.squares.cpu(), ref.squares) and torch.equal(env.turn.cpu(), ref.turn)
    assert not torch.equal(seen[0]["visits"], seen[1]["visits"]) and not torch.equal(seen[0]["actions"], seen[1]["actions"])
