"""gbl_evaluate / gbl_tree_search_eval on the MI355X (-m gpu): k_evaluate and k_tree_eval against the host flavour and the Python
restatement of the header text, bit for bit, with canaries around every output, NULL optional outputs, every hidden size, the tree
sizes 1 / 2 / 64 / 512 and a batch beyond the grid cap.  (k_tree_eval has one instantiation -- one wavefront per board at every
batch size -- so the batch sizes are those of a wavefront's edges: 1, 3, 65 boards, and 4097.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from tests import evaluator_restatement as R
from tests.selfplay_harness import DeviceNet
from tests.test_playout_policy import UNCOVER_SEQ, WIN_SEQ, play

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
THREADS = 16
GRID_CAP = 1 << 20
CANARY = 5  # elements of -7 / 99 kept before and after every output


@pytest.fixture(scope="module")
def G():
    import gobblet_rl_amd as g
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    g._native.lib()
    g._native.cpu_raw().gbl_cpu_set_threads(THREADS)
    return g


@pytest.fixture(scope="module")
def c5(G):
    env = G.BatchedGobblet(65536, DEV, auto_reset=True, seed=11)
    env.rollout(64)
    torch.cuda.synchronize()
    st, tm = env.squares.cpu().numpy().copy(), env.to_move.cpu().numpy().copy()
    assert (oracle.batch_winner(st) == 0).all() and 0.3 < tm.mean() < 0.7
    (sw, mw), (su, mu) = play(WIN_SEQ), play(UNCOVER_SEQ)  # boards 1 and 2: roots one move from a decided game
    st[1], tm[1], st[2], tm[2] = sw, mw, su, mu
    return st, tm


def guarded(n, width, dtype, fill):
    """An output of n rows with CANARY rows of `fill` on either side: (whole tensor, pointer of row 0)."""
    shape = (n + 2 * CANARY, width) if width else (n + 2 * CANARY,)
    t = torch.full(shape, fill, dtype=dtype, device=DEV)
    return t, t[CANARY:].data_ptr()


def unguard(t, n, fill):
    a = t.cpu().numpy()
    assert (a[:CANARY] == fill).all() and (a[CANARY + n:] == fill).all(), "an output was written outside its rows"
    return a[CANARY:CANARY + n]


def device_evaluate(G, dnet, st, tm, mask=None, logits=True):
    nat = G._native
    n = len(st)
    d_st, d_tm = torch.from_numpy(np.ascontiguousarray(st)).to(DEV), torch.from_numpy(np.ascontiguousarray(tm)).to(DEV)
    d_mk = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    pri, p_pri = guarded(n, 54, torch.uint8, 99)
    val, p_val = guarded(n, 0, torch.int32, -7)
    log, p_log = guarded(n, 56, torch.int32, -7)
    ev = dnet.struct()
    nat.check(nat.lib().gbl_evaluate(d_st.data_ptr(), d_tm.data_ptr(), nat.ptr(d_mk), C.addressof(ev), p_pri, p_val, p_log if logits else None,
                                     n, nat.current_stream(DEV)), "gbl_evaluate")
    torch.cuda.synchronize()
    out_log = unguard(log, n, -7)
    if not logits:
        assert (out_log == -7).all()
    return unguard(pri, n, 99), unguard(val, n, -7), out_log if logits else None


def device_search(G, dnet, st, tm, mask, iterations, explore, keep=R.SEARCH_NAMES):
    """gbl_tree_search_eval with only the outputs named in `keep` given: {name: array}."""
    nat = G._native
    n = len(st)
    d_st, d_tm = torch.from_numpy(np.ascontiguousarray(st)).to(DEV), torch.from_numpy(np.ascontiguousarray(tm)).to(DEV)
    d_mk = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV)
    bufs = {}
    for k in keep:
        if k == "root_priors":
            bufs[k] = guarded(n, 54, torch.uint8, 99) + (99,)
        else:
            bufs[k] = guarded(n, 54 if k in ("visits", "wins", "losses") else 0, torch.int32, -7) + (-7,)
    ev = dnet.struct()
    nat.check(nat.lib().gbl_tree_search_eval(d_st.data_ptr(), d_tm.data_ptr(), nat.ptr(d_mk), C.addressof(ev), iterations, explore,
                                             *[bufs[k][1] if k in bufs else None for k in R.SEARCH_NAMES], n, nat.current_stream(DEV)),
              "gbl_tree_search_eval")
    torch.cuda.synchronize()
    return {k: unguard(t, n, fill) for k, (t, _, fill) in bufs.items()}


def host_search(G, net, st, tm, mask, iterations, explore):
    return dict(zip(R.SEARCH_NAMES, R.run_search(G._native.cpu_raw(), net, st, tm, mask, iterations, explore)))


def same_dict(got, exp):
    for k in got:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (k, np.argwhere(got[k] != exp[k])[:5])


def kinds(hidden):
    return {"random": R.random_net(hidden, 5 + hidden), "max": R.extreme_net(hidden, 1, 1), "mixed": R.extreme_net(hidden, 1, -1),
            "min": R.extreme_net(hidden, -1, -1), "zero": R.zero_net(hidden)}


@pytest.mark.parametrize("hidden", [64, 128, 192, 256])
def test_k_evaluate_equals_host_flavour_and_restatement(G, c5, hidden):
    cpu = G._native.cpu_raw()
    for kind, net in kinds(hidden).items():
        dnet = DeviceNet(net)
        for n in (1, 3, 65, 4097):
            st, tm = c5[0][:n], c5[1][:n]
            mask = (np.random.default_rng(n).random((n, 54)) < 0.4).astype(np.int8)
            mask[0] = 0
            for mk in (None, mask):
                got = device_evaluate(G, dnet, st, tm, mk)
                R.same(got, R.run_evaluate(cpu, net, st, tm, mk), R.EVAL_NAMES)
                if n <= 65:
                    R.same(got, R.restate_evaluate(net, st, tm, mk), R.EVAL_NAMES)
            assert np.array_equal(device_evaluate(G, dnet, st, tm, mask, logits=False)[0], got[0])  # (logits_out NULL)


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
        got = device_search(G, dnet, st, tm, mask, iterations, explore)
        exp = host_search(G, net, st, tm, mask, iterations, explore)
        same_dict(got, exp)
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
        got = device_search(G, dnet, st, tm, mask, iterations, explore)
        same_dict(got, dict(zip(R.SEARCH_NAMES, R.restate_search(net, st, tm, mask, iterations, explore))))


def test_null_optional_outputs(G, c5):
    net = R.random_net(128, 1)
    dnet = DeviceNet(net)
    st, tm = c5[0][:130], c5[1][:130]
    full = device_search(G, dnet, st, tm, None, 48, 64)
    for keep in (("action",), ("visits", "root_value"), ("wins", "losses", "nodes", "root_priors"), ()):
        got = device_search(G, dnet, st, tm, None, 48, 64, keep)
        assert set(got) == set(keep)
        same_dict(got, full)


def test_beyond_the_grid_cap(G, c5):
    """2^20 + 65 boards: the grid-stride loops' second trip runs on 65 workgroups, and must keep nothing of the first trip's trees."""
    n = GRID_CAP + 65
    st, tm = np.resize(c5[0], (n, 27)), np.resize(c5[1], n)
    net = R.random_net(64, 7)
    dnet = DeviceNet(net)
    got = device_search(G, dnet, st, tm, None, 2, 64, ("visits", "action", "nodes", "root_value"))
    head = host_search(G, net, st[:65536], tm[:65536], None, 2, 64)
    for k in got:  # (the batch is the 65 536 boards over and over, and a board's search depends on the board alone)
        assert np.array_equal(got[k], np.resize(head[k], got[k].shape)), k
    pri, val, _ = device_evaluate(G, dnet, st, tm, None, logits=False)
    hp, hv, _ = R.run_evaluate(G._native.cpu_raw(), net, st[:65536], tm[:65536], None, logits=False)
    assert np.array_equal(pri, np.resize(hp, pri.shape)) and np.array_equal(val, np.resize(hv, val.shape))


def test_policy_on_device(G, c5):
    net = R.random_net(64, 3)
    ev = G.GobbletEvaluator(net.w1, net.b1, net.w2, net.b2, net.shift1, net.shift_p, net.shift_v, device=DEV)
    st, tm = torch.from_numpy(c5[0][:256]).to(DEV), torch.from_numpy(c5[1][:256]).to(DEV)
    pol = G.EvaluatorTreeSearchGobbletPolicy(ev, iterations=100)
    a = pol.compute_actions_from_state(st, tm)
    exp = host_search(G, net, c5[0][:256], c5[1][:256], None, 100, pol.explore)
    last = dict(visits=pol.last_visits, wins=pol.last_wins, losses=pol.last_losses, action=pol.last_action, nodes=pol.last_nodes,
                root_value=pol.last_root_value, root_priors=pol.last_root_priors)
    assert a.device.type == "cuda" and all(t.device.type == "cuda" for t in last.values())
    same_dict({k: v.cpu().numpy() for k, v in last.items()}, exp)
    pri, val = ev.evaluate(st, tm)
    cp, cv = ev.to("cpu").evaluate(st.cpu(), tm.cpu())
    assert torch.equal(pri.cpu(), cp) and torch.equal(val.cpu(), cv)
