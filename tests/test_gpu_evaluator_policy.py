"""gbl_evaluate / gbl_tree_search_eval on the MI355X (-m gpu): k_evaluate and k_tree_eval against the host flavour and the Python
restatement of the header text, bit for bit, with canaries around every output, NULL optional outputs, every hidden size, the tree
sizes 1 / 2 / 64 / 512 and a batch beyond the grid cap.  (k_tree_eval has one instantiation -- one wavefront per board at every
batch size -- so the batch sizes are those of a wavefront's edges: 1, 3, 65 boards, and 4097.)"""
import numpy as np
import pytest
import torch

from tests import evaluator_restatement as R
from tests.search_harness import DEV, G, midgame_boards, run, same  # noqa: F401  (G: the fixture)
from tests.selfplay_harness import DeviceNet

pytestmark = pytest.mark.gpu

GRID_CAP = 1 << 20


@pytest.fixture(scope="module")
def c5(G):
    return midgame_boards(planted=True)  # boards 1 and 2: roots one move from a decided game


def kinds(hidden):
    return {"random": R.random_net(hidden, 5 + hidden), "max": R.extreme_net(hidden, 1, 1), "mixed": R.extreme_net(hidden, 1, -1),
            "min": R.extreme_net(hidden, -1, -1), "zero": R.zero_net(hidden)}


@pytest.mark.parametrize("hidden", [64, 128, 192, 256])
def test_k_evaluate_equals_host_flavour_and_restatement(G, c5, hidden):
    for kind, net in kinds(hidden).items():
        dnet = DeviceNet(net)
        for n in (1, 3, 65, 4097):
            st, tm = c5[0][:n], c5[1][:n]
            mask = (np.random.default_rng(n).random((n, 54)) < 0.4).astype(np.int8)
            mask[0] = 0
            for mk in (None, mask):
                got = run("evaluate", DEV, st, tm, mk, (), dnet)
                same(got, run("evaluate", "cpu", st, tm, mk, (), net))
                if n <= 65:
                    same(got, R.restate_evaluate(net, st, tm, mk))
            assert np.array_equal(run("evaluate", DEV, st, tm, mask, (), dnet, keep=("priors", "value"))["priors"], got["priors"])  # (logits_out NULL)


@pytest.mark.parametrize("hidden", [64, 128, 192, 256])
@pytest.mark.parametrize("iterations", [1, 2, 64, 512])
def test_k_tree_eval_equals_host_flavour(G, c5, hidden, iterations):
    net = R.random_net(hidden, 5 + hidden)
    dnet = DeviceNet(net)
    for n, explore in ((1, 64), (3, 0), (65, 1024), (4097 if iterations <= 64 else 257, 64)):
        st, tm = c5[0][:n], c5[1][:n]
        mask = None
        if n == 65:
            mask = (np.random.default_rng(n).random((n, 54)) < 0.4).astype(np.int8)
            mask[0] = 0  # a board without a candidate
        got = run("tree_search_eval", DEV, st, tm, mask, (iterations, explore), dnet)
        exp = run("tree_search_eval", "cpu", st, tm, mask, (iterations, explore), net)
        same(got, exp)
        assert (got["visits"].sum(1)[got["action"] >= 0] == iterations).all() and (got["nodes"] <= iterations + 1).all()
        if mask is not None:
            assert got["action"][0] == -1 and got["nodes"][0] == 1 and not got["root_priors"][0].any()


@pytest.mark.parametrize("kind,hidden", [("random", 64), ("random", 256), ("zero", 128), ("mixed", 192), ("max", 64), ("min", 256)])
def test_k_tree_eval_equals_restatement(G, c5, kind, hidden):
    net = kinds(hidden)[kind]
    dnet = DeviceNet(net)
    st, tm = c5[0][:6], c5[1][:6]
    mask = np.ones((6, 54), np.int8)
    mask[3] = 0
    mask[4, 27:] = 0
    for iterations, explore in ((1, 64), (2, 1024), (64, 64), (200, 16)):
        got = run("tree_search_eval", DEV, st, tm, mask, (iterations, explore), dnet)
        same(got, R.restate_search(net, st, tm, mask, iterations, explore))


def test_null_optional_outputs(G, c5):
    net = R.random_net(128, 1)
    dnet = DeviceNet(net)
    st, tm = c5[0][:130], c5[1][:130]
    full = run("tree_search_eval", DEV, st, tm, None, (48, 64), dnet)
    for keep in (("action",), ("visits", "root_value"), ("wins", "losses", "nodes", "root_priors"), ()):
        got = run("tree_search_eval", DEV, st, tm, None, (48, 64), dnet, keep)
        assert set(got) == set(keep)
        same(got, full)


def test_beyond_the_grid_cap(G, c5):
    """2^20 + 65 boards: the grid-stride loops' second trip runs on 65 workgroups, and must keep nothing of the first trip's trees."""
    n = GRID_CAP + 65
    st, tm = np.resize(c5[0], (n, 27)), np.resize(c5[1], n)
    net = R.random_net(64, 7)
    dnet = DeviceNet(net)
    got = run("tree_search_eval", DEV, st, tm, None, (2, 64), dnet, ("visits", "action", "nodes", "root_value"))
    head = run("tree_search_eval", "cpu", st[:65536], tm[:65536], None, (2, 64), net)
    for k in got:  # (the batch is the 65 536 boards over and over, and a board's search depends on the board alone)
        assert np.array_equal(got[k], np.resize(head[k], got[k].shape)), k
    pri, val = run("evaluate", DEV, st, tm, None, (), dnet, ("priors", "value")).values()
    hp, hv = run("evaluate", "cpu", st[:65536], tm[:65536], None, (), net, ("priors", "value")).values()
    assert np.array_equal(pri, np.resize(hp, pri.shape)) and np.array_equal(val, np.resize(hv, val.shape))


def test_policy_on_device(G, c5):
    net = R.random_net(64, 3)
    ev = G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, net.shift1, net.shift_p, net.shift_v, device=DEV)
    st, tm = torch.from_numpy(c5[0][:256]).to(DEV), torch.from_numpy(c5[1][:256]).to(DEV)
    pol = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=100)
    a = pol.compute_actions_from_state(st, tm)
    exp = run("tree_search_eval", "cpu", c5[0][:256], c5[1][:256], None, (100, pol.explore), net)
    last = dict(visits=pol.last_visits, wins=pol.last_wins, losses=pol.last_losses, action=pol.last_action, nodes=pol.last_nodes,
                root_value=pol.last_root_value, root_priors=pol.last_root_priors)
    assert a.device.type == "cuda" and all(t.device.type == "cuda" for t in last.values())
    same({k: v.cpu().numpy() for k, v in last.items()}, exp)
    pri, val = ev.evaluate(st, tm)
    cp, cv = ev.to("cpu").evaluate(st.cpu(), tm.cpu())
    assert torch.equal(pri.cpu(), cp) and torch.equal(val.cpu(), cv)
