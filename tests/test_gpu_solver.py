"""gbl_solve on the MI355X (-m gpu): k_solve against the host flavour byte for byte (which tests/test_solver.py holds to the
restatement of the contract), canaries, NULL outputs, a side stream, a captured graph, the argument errors, and the Python surface on
the device."""
import functools

import numpy as np
import pytest
import torch

from tests import solver_restatement as R
from tests.search_harness import DEV, SOLVE_NAMES, Call, G, run, same  # noqa: F401  (G: the fixture)
from tests.solver_restatement import DEEP, hand_built, sample

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def boards65():
    """65 boards: the hand-built pair first (so that 1 and 3 boards hold them), then a board with player_2 to move, the rest of the
    restatement tests' sample, and late positions."""
    st, tm = sample()
    more = R.rollout_positions(12, seed=5)
    order = np.array([len(st) - 2, len(st) - 1, 3] + [i for i in range(len(st) - 2) if i != 3])
    st = np.concatenate([st[order], more[0][-12:]])
    tm = np.concatenate([tm[order], more[1][-12:]])
    assert len(st) == 65 and tm[:3].min() == 0 and tm[:3].max() == 1  # both sides to move, in the smallest ragged batch too
    return np.ascontiguousarray(st), np.ascontiguousarray(tm)


def masks(n):
    m = (np.random.default_rng(4).random((n, 54)) < 0.6).astype(np.int8) * np.int8(-2)  # (set = non-zero)
    m[n // 2] = 0  # a root without a candidate
    return m


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_device_equals_host_flavour(G, n, with_mask):
    st, tm = (a[:n] for a in boards65())
    mask = masks(n) if with_mask else None
    for depth in (1, 2, 3, 4):
        same(run("solve", DEV, st, tm, mask, (depth,), misaligned=True), run("solve", "cpu", st, tm, mask, (depth,)))


@pytest.mark.parametrize("depth", [5, 6])
def test_deep_searches_of_late_positions(G, depth):
    pool = R.rollout_positions(120, seed=3)
    st, tm = (np.ascontiguousarray(a[np.array(DEEP)]) for a in pool)
    exp = run("solve", "cpu", st, tm, None, (depth,))
    same(run("solve", DEV, st, tm, None, (depth,), misaligned=True), exp)
    assert (np.abs(exp["value"]) == depth).any() or depth == 5 and (exp["value"] == 5).any()


def test_zugzwang_boards(G):
    """The hand-built boards with a win in two beside a win in three (solver_restatement.zugzwang; tests/test_solver.py holds the
    host flavour to the restatement on them): the node as a root, at the reply level where the lanes share its key, and one ply
    deeper inside a lane's recursion; with the mask that leaves only the way to the node, too."""
    st, tm = (a.copy() for a in R.zugzwang())
    only = np.zeros((3, 54), np.int8)
    only[0, R.ZUG_ROOT_ACTION] = only[1, R.ZUG_WIN_IN_2] = only[1, R.ZUG_WIN_IN_3] = only[2, R.ZUG_DEEP_ACTIONS[0]] = 1
    for mask in (None, only):
        for depth in (3, 4, 5, 6):
            exp = run("solve", "cpu", st, tm, mask, (depth,))
            same(run("solve", DEV, st, tm, mask, (depth,), misaligned=True), exp)
    out = exp["outcome"]
    assert out[0, R.ZUG_ROOT_ACTION] == -3 and out[1, R.ZUG_WIN_IN_2] == 2 and out[2, R.ZUG_DEEP_ACTIONS[0]] == 4


def test_null_outputs_and_a_side_stream(G):
    st, tm = (a[:3] for a in boards65())
    exp = run("solve", "cpu", st, tm, None, (3,))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for skip in SOLVE_NAMES:
            call = Call("solve", DEV, keep=[k for k in SOLVE_NAMES if k != skip], misaligned=True).load(st, tm)
            call.launch((3,))
            side.synchronize()
            got = call.results()
            assert skip not in got and len(got) == 2
            same(got, exp)
    torch.cuda.current_stream().wait_stream(side)


def test_replay_from_a_captured_graph(G):
    st, tm = boards65()
    sets = [(st[:33], tm[:33]), (np.ascontiguousarray(st[32:]), np.ascontiguousarray(tm[32:]))]
    call = Call("solve", DEV, misaligned=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.load(*sets[0])
        call.launch((3,))  # warm-up on the side stream
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            call.launch((3,))
        for s, t in sets:
            call.load(s, t)  # in place: the captured launch holds these addresses
            g.replay()
            side.synchronize()
            same(call.results(), run("solve", "cpu", s, t, None, (3,)))
    torch.cuda.current_stream().wait_stream(side)


def test_argument_errors(G):
    nat = G._native
    L = nat.lib()
    solve = L.gbl_solve
    st, tm = (torch.from_numpy(a).to(DEV) for a in hand_built())
    out = torch.zeros((2, 54), dtype=torch.int8, device=DEV)
    val = torch.zeros(2, dtype=torch.int8, device=DEV)
    act = torch.zeros(3, dtype=torch.int32, device=DEV)
    odd = act.data_ptr() + 1

    def call(state, to_move, depth, action, n):
        rc = solve(state, to_move, None, depth, out.data_ptr(), val.data_ptr(), action, n, None)
        return rc, L.gbl_last_error().decode()
    assert call(None, None, 0, odd, -1) == (nat.ERR_ARG, "n < 0")
    assert call(None, None, 0, odd, 0) == (nat.ERR_ARG, "depth must be in [1, 6]")
    assert call(st.data_ptr(), tm.data_ptr(), 7, act.data_ptr(), 2) == (nat.ERR_ARG, "depth must be in [1, 6]")
    assert call(None, None, 6, odd, 0)[0] == nat.OK
    assert call(None, None, 1, odd, 2) == (nat.ERR_ARG, "state must not be NULL")
    assert call(st.data_ptr(), None, 1, odd, 2) == (nat.ERR_ARG, "to_move must not be NULL")
    assert call(st.data_ptr(), tm.data_ptr(), 1, odd, 2) == (nat.ERR_ALIGN, "action_out must be 4-byte aligned")
    assert call(st.data_ptr(), tm.data_ptr(), 1, act.data_ptr(), 2)[0] == nat.OK
    torch.cuda.synchronize()


def test_policy_and_env_on_the_device(G):
    st, tm = boards65()
    tree = [G.TreeSearchGobbletPolicy(iterations=8, playouts=2, device=d) for d in (DEV, "cpu")]
    for fb in (None, tree):
        gpu, cpu = (G.SolverGobbletPolicy(3, device=d, fallback=None if fb is None else fb[i]) for i, d in enumerate((DEV, "cpu")))
        a_gpu = gpu.compute_actions_from_state(torch.from_numpy(st).to(DEV), torch.from_numpy(tm).to(DEV))
        a_cpu = cpu.compute_actions_from_state(st.copy(), tm.copy())
        assert a_gpu.device.type == "cuda" and torch.equal(a_gpu.cpu(), a_cpu)
        assert torch.equal(gpu.last_outcomes.cpu(), cpu.last_outcomes) and torch.equal(gpu.last_value.cpu(), cpu.last_value)
    assert torch.equal(gpu.outcomes(st.copy(), tm.copy()).cpu(), cpu.last_outcomes)
    envs = []
    for d in (DEV, "cpu"):
        env = G.BatchedGobblet(65, d)
        env.squares.copy_(torch.from_numpy(st))
        env.to_move.copy_(torch.from_numpy(tm))
        envs.append(env.solve(3))
    for k in ("outcome", "value", "action"):
        assert torch.equal(envs[0][k].cpu(), envs[1][k]), k
    assert torch.equal(envs[1]["outcome"], cpu.last_outcomes)
