"""The integer evaluator's edges on the MI355X (-m gpu): the dial networks and shift triples of tests/test_evaluator_edges.py through
k_evaluate and k_tree_eval with canaried outputs at 1, 3 and 65 boards, the float64 reference once more through the device, the two
entry points replayed from a captured graph with weights and boards refreshed in place.  (No performance guard yet: a guard's ceiling
is read from a device record of scripts/bench_evaluator_policy.py, and profiles/r10/evaluator_policy.json has no timing rows.)"""
import numpy as np
import pytest
import torch

from tests import evaluator_restatement as R
from tests.test_evaluator_edges import SHIFT_TRIPLES, TOPS, compare_with_float, dial_cases, float_weights, midgame, search_dial  # noqa: F401
from tests.search_harness import DEV, Call, G, run, same  # noqa: F401  (G: the fixture)
from tests.selfplay_harness import DeviceNet
from tests.test_gpu_evaluator_policy import c5  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 65)


def on_device_equals_both(G, net, st, tm, mask, sizes=SIZES):
    """k_evaluate at every size (the boards repeated) against the restatement and the host flavour of the boards themselves."""
    exp = R.restate_evaluate(net, st, tm, mask)
    same(run("evaluate", "cpu", st, tm, mask, (), net), exp)
    dnet = DeviceNet(net)
    for n in sizes:
        idx = np.arange(n) % len(st)
        got = run("evaluate", DEV, st[idx], tm[idx], None if mask is None else mask[idx], (), dnet)
        same(got, [e[idx] for e in exp])
    return exp


def test_logit_dials_on_device(G, midgame):
    """Every distance of the table's edges on every lane position of the largest logit (the closed forms are asserted on the
    restatement in tests/test_evaluator_edges.py; here the kernel must give the restatement's bytes)."""
    for top, rot, sp, low in dial_cases():
        st, tm, mask = R.dial_boards(midgame, top)
        on_device_equals_both(G, R.distance_dial(top, rot, sp, low)[0], st, tm, mask, SIZES if rot == 0 else (65,))
    for top in TOPS:
        st, tm, mask = R.dial_boards(midgame, top)
        logit = np.full(54, -(1 << 24), np.int64)
        logit[top] = 1 << 24
        pri = on_device_equals_both(G, R.logit_dial(logit), st, tm, mask)[0]
        assert pri[0, top] == 254 and pri[5].max() == 255


def test_value_hidden_and_floor_dials_on_device(G):
    st, tm = np.zeros((2, 27), np.int8), np.array([0, 1], np.int8)
    for shift_v in (0, 7):
        for raw in (-129, -128, -127, -1, 0, 127, 128, 129):
            val = on_device_equals_both(G, R.value_dial(raw, shift_v, (1 << shift_v) - 1), st, tm, None)[1]
            assert (val == min(max(raw, -128), 128)).all()
    for shift1 in (0, 5, 13):
        values = [v for v in (-2, -1, 0, 1, 126, 127, 128, 300) if abs(v) << shift1 <= 1 << 20]
        raw = np.array([values[(j + 3) % len(values)] for j in range(64)])
        log = on_device_equals_both(G, R.hidden_dial(raw, shift1), st, tm, None)[2]
        assert np.array_equal(log[0, :54], np.clip(raw[:54], 0, 127))
    for b1 in (1 << 20, -(1 << 20)):
        net = R.hidden_dial(np.zeros(64, np.int64), 24)
        net.b1[:] = b1
        assert (on_device_equals_both(G, net, st, tm, None)[2] == 0).all()
    b2 = np.zeros(56, np.int32)
    b2[1::2] = -1
    b2[54] = -1
    mask = np.zeros((2, 54), np.int8)
    mask[0], mask[1, :2] = 1, 1
    pri, val, _ = on_device_equals_both(G, R._dial(b2=b2, shift_p=24, shift_v=24), st, tm, mask)
    assert (val == -1).all() and pri[1, 0] == 130 and pri[1, 1] == 125


def test_search_on_a_logit_dial_on_device(G, midgame):
    """explore = 1024, 512 iterations, a root with one candidate (prior 255) and a root with all 54: the largest selection key."""
    top = 26
    st, tm, mask = R.dial_boards(midgame, top)
    st, tm, mask = st[[5, 0]], tm[[5, 0]], mask[[5, 0]]
    net = search_dial(top)
    exp = run("tree_search_eval", "cpu", st, tm, mask, (512, 1024), net)
    same(exp, R.restate_search(net, st, tm, mask, 512, 1024))
    dnet = DeviceNet(net)
    for n in SIZES:
        idx = np.arange(n) % 2
        same(run("tree_search_eval", DEV, st[idx], tm[idx], mask[idx], (512, 1024), dnet), {k: v[idx] for k, v in exp.items()})
    assert exp["root_priors"][0].max() == 255 and exp["visits"][0, top] == 512


@pytest.mark.parametrize("hidden", [64, 256])
@pytest.mark.parametrize("shifts", SHIFT_TRIPLES)
def test_shift_sweep_on_device(G, c5, hidden, shifts):
    st, tm = c5[0][:65], c5[1][:65]
    net = R.random_net(hidden, 40 + hidden, *shifts)
    mask = (np.random.default_rng(7).random((65, 54)) < 0.5).astype(np.int8)
    for mk in (None, mask):
        on_device_equals_both(G, net, st, tm, mk, (65,))
    low, high, mid = R.hidden_census(net, st, tm)
    print("shifts %s H %d: hidden units clamped at 0: %d, at 127: %d, in between: %d" % (shifts, hidden, low, high, mid))
    # |sum| <= 300 + 21 * 128 = 2988: >> 24 leaves 0 or -1, >> 7 at most 23; unshifted, sums of a few hundred reach 127
    assert (low == 65 * hidden) == (shifts[0] == 24) and (mid > 0) == (shifts[0] != 24)
    assert high == 0 if shifts[0] >= 7 else (high > 0 or shifts[0] == 3)
    got = run("tree_search_eval", DEV, st, tm, mask, (48, 16), DeviceNet(net))
    same(got, run("tree_search_eval", "cpu", st, tm, mask, (48, 16), net))
    if hidden == 64:
        same(got, R.restate_search(net, st, tm, mask, 48, 16))


def test_dequantised_weights_against_the_float_reference_on_device(G, c5):
    """Comparison (a) of tests/test_evaluator_edges.py through GobbletEvaluator(..., device="cuda:0").evaluate: 65 boards, H = 256."""
    st, tm = np.ascontiguousarray(c5[0][:65]), np.ascontiguousarray(c5[1][:65])
    cpu_ev = G.GobbletEvaluator.from_float(*float_weights(256, 1))
    ev = cpu_ev.to(DEV)
    assert ev.w1.device.type == "cuda" and ev.scales == cpu_ev.scales
    compare_with_float(cpu_ev, R.dequantised(cpu_ev), st, tm, rounding=False, evaluate=lambda s, m: ev.evaluate(s.to(DEV), m.to(DEV)))


# ---- stream and graph use ---------------------------------------------------------------------------------------------------------
class Session:
    """The two entry points on fixed device tensors: what a training loop keeps between weight refreshes."""

    def __init__(self, net, iterations, explore):
        self.net, self.params = net, (iterations, explore)
        self.arrays = [torch.empty_like(torch.from_numpy(a), device=DEV) for a in (net.w1, net.b1, net.w2, net.b2)]
        self.calls = [Call("evaluate", DEV, self), Call("tree_search_eval", DEV, self)]

    def struct(self):
        return self.net.struct(self.arrays)

    def load(self, net, st, tm):
        """copy_ into the SAME tensors, on the current stream (the shifts are launch arguments: a refreshed network keeps them);
        every output is filled anew."""
        assert (net.shift1, net.shift_p, net.shift_v, net.hidden) == (self.net.shift1, self.net.shift_p, self.net.shift_v, self.net.hidden)
        for dst, src in zip(self.arrays, (net.w1, net.b1, net.w2, net.b2)):
            dst.copy_(torch.from_numpy(src), non_blocking=False)
        for call in self.calls:
            call.load(st, tm)

    def launch(self):
        self.calls[0].launch()
        self.calls[1].launch(self.params)

    def check(self, net, st, tm):
        same(self.calls[0].results(), run("evaluate", "cpu", st, tm, None, (), net))
        same(self.calls[1].results(), run("tree_search_eval", "cpu", st, tm, None, self.params, net))


def test_graph_replay_with_weights_and_boards_refreshed_in_place(G, c5):
    """gbl_evaluate then gbl_tree_search_eval captured on a side stream (one linear chain), replayed, then replayed again after copy_
    of another network's arrays and other boards into the same tensors; and the same two calls uncaptured on the side stream with
    inputs produced on it."""
    n, I = 65, 16
    nets = [R.random_net(64, s, 3, 5, 12) for s in (71, 72)]
    boards = [(np.ascontiguousarray(c5[0][o:o + n]), np.ascontiguousarray(c5[1][o:o + n])) for o in (0, 300)]
    ses = Session(nets[0], I, 16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ses.load(nets[0], *boards[0])
        ses.launch()  # warm-up on the side stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            ses.launch()
        for net, (st, tm) in zip(nets, boards):
            ses.load(net, st, tm)
            g.replay()
            side.synchronize()
            ses.check(net, st, tm)
        # uncaptured, inputs produced on the side stream: the second network on the first boards
        ses.load(nets[1], *boards[0])
        ses.launch()
        side.synchronize()
        ses.check(nets[1], *boards[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
