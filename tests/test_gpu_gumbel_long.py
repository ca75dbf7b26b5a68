"""The Gumbel root rule's wave-level code on the MI355X where tests/test_gpu_gumbel_search.py does not take it (-m gpu): chains of three
and four halvings (tests/gumbel_harness.py::LONG_PAIRS and (16, 64): 54 -> 27 -> 14 -> 7 -> 4 -> 2 over 512 iterations among them), the
rule's three arithmetic edges through the wave_max / wave_sum butterflies, self-play at budgets up to 512, and a launch of more boards
than the grid has workgroups (2^20 + 65), so that the per-board re-initialisation of the rule's wave state in the grid-stride loop is
seen.  The reference is the host flavour throughout (pinned to the restatement of the header's text in tests/test_gumbel_search.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests.gumbel_harness import (LONG_PAIRS, device_collect_gumbel, host_collect_gumbel, root_value_edge_case, rule_boards, sigma_edge_case,
                                  winning_action_case)
from tests.search_harness import DEV, ENTRIES, G, run  # noqa: F401  (G: the fixture)
from tests.search_harness import same as same_arrays
from tests.selfplay_harness import EVAL_NAMES, DeviceNet, call_args, same, strides
from tests.test_gumbel_search import SCHEDULE
from tests.test_selfplay_solve import EXPLORE, fixture_boards, smoke_net

pytestmark = pytest.mark.gpu

GUMBEL = "tree_search_gumbel"
SEED, ENV_BASE = 0xFEDCBA9876543210, (1 << 41) + 77
COMBOS = ((0, 0), (1, 23), (1, 64))  # (gumbel_noise, scale)
BIG = (1 << 20) + 65                 # boards of the launches that go round the grid-stride loop twice: the grid has 2^20 workgroups


@pytest.fixture(scope="module")
def roots(G):
    """130 roots: the first two empty (54 candidates), the last eight under masks of 27, 2, 1 and 0 candidates."""
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
    """(host nets, device nets): H = 64 and 128."""
    pair = (smoke_net(), R.random_net(128, 77))
    return pair, tuple(DeviceNet(x) for x in pair)


@pytest.fixture(scope="module")
def reference(roots, nets):
    """The host flavour on the 130 roots, once per (pair, noise, scale, net).  The smaller launches run the LAST boards under
    env_base + 130 - n: a board keeps its id, and with it its Gumbel row, so their reference is a slice of this one."""
    done = {}

    def get(pair, noise, scale, k):
        key = (pair, noise, scale, k)
        if key not in done:
            done[key] = run(GUMBEL, "cpu", *roots, (pair[1], EXPLORE, pair[0], noise, 50, scale, SEED, ENV_BASE, 5), nets[0][k])
        return done[key]
    return get


# ---- 1. the long schedules ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", LONG_PAIRS + ((16, 64),))
@pytest.mark.parametrize("n", [1, 65, 130])
def test_k_tree_gumbel_long_schedules_equal_host_flavour(G, roots, nets, reference, n, pair):
    st, tm, mask = (x[-n:] for x in roots)
    considered, iterations = pair
    for noise, scale in COMBOS:
        for k in (0, 1):
            exp = reference(pair, noise, scale, k)
            got = run(GUMBEL, DEV, st, tm, mask, (iterations, EXPLORE, considered, noise, 50, scale, SEED, ENV_BASE + 130 - n, 5), nets[1][k])
            same_arrays(got, {x: v[-n:] for x, v in exp.items()})
            if n < 130:
                continue
            # the halvings happened: the roots of 54 candidates follow the schedule worked out by hand, and nearly every root ends on two actions
            rows = -np.sort(-got["visits"][:2], axis=1)[:, :considered]
            assert mask[:2].all() and (rows == np.array(SCHEDULE[pair])).all()
            two = ((got["visits"] > iterations // 8).sum(1) == 2).sum()
            print("%s noise %d scale %d H %d: %d of 130 roots end on two actions" % (pair, noise, scale, nets[0][k].hidden, two))
            assert two >= 100


# ---- 2. the rule's arithmetic edges ----------------------------------------------------------------------------------------------------------
def on_both(case):
    """A case of tests/gumbel_harness.py on the device: equal to the host flavour, and the closed-form expectation on the kernel's own bytes."""
    (st, tm), mask, net, params, expect = case
    got = run(GUMBEL, DEV, st, tm, mask, params, DeviceNet(net))
    same_arrays(got, run(GUMBEL, "cpu", st, tm, mask, params, net))
    expect(got)
    return got


def test_sigma_at_its_largest_stays_inside_uint32_on_the_device(G):
    """(255 + 512) * 64 * 65536 >= 2^31 through wave_max and the lane's multiply: sigma = 49 088, the floor byte on every other action."""
    on_both(sigma_edge_case())


@pytest.mark.parametrize("q_raw", [-128, -37, 0, 90, 128])
def test_an_unvisited_action_uses_the_root_value_on_the_device(G, q_raw):
    for vo, scale in ((50, 23), (0, 64), (255, 1)):
        on_both(root_value_edge_case(q_raw, vo, scale))


def test_an_action_that_wins_at_once_is_decided_whenever_it_is_considered_on_the_device(G):
    on_both(winning_action_case(SEED, ENV_BASE))


# ---- 3. self-play at long budgets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("its,considered", [((64, 512), (16, 54)), ((200, 96), (27, 7))])
def test_k_collect_gumbel_long_budgets_equal_host_flavour(G, boards, nets, its, considered):
    """most = 512: (512 + 1) * 72 bytes of dynamic LDS beside the row images."""
    hn, dn = nets
    st, tm, turn = (x[:65] for x in boards)
    for layout, noise, scale in (("time", 1, 23), ("tile", 1, 64)):
        kw = dict(noise=noise, scale=scale, X=EXPLORE, sample_plies=4, layout=layout, seed=SEED, env_base=ENV_BASE, ply0=3)
        got = device_collect_gumbel(st, tm, turn, 4, ("eval", "eval"), dn, its, considered, **kw)
        same(got, host_collect_gumbel(st, tm, turn, 4, ("eval", "eval"), hn, its, considered, **kw))
        rows = got[0]["visits"]
        assert (got[0]["how"] == nat.HOW_GUMBEL).all() and rows.max() <= 255 and (rows.sum(-1) >= 255).all()
        assert {0, 1} == set(np.unique(got[0]["mover"]).tolist())  # (both budgets ran)


# ---- 4. a second trip through the grid-stride loop ------------------------------------------------------------------------------------------------
def cycled(arrays, lo, hi):
    """Boards lo .. hi - 1 of the launch whose board b is root b % 130."""
    at = np.arange(lo, hi) % 130
    return [np.ascontiguousarray(x[at]) for x in arrays]


def test_k_tree_gumbel_more_boards_than_workgroups(G, roots, nets):
    """2^20 + 65 boards, 2 iterations, considered 2, noise on: workgroups 0 .. 64 search a second board, 2^20 + their first one.  The first
    64 and the last 130 boards equal the host flavour's launches on those boards under their own board ids."""
    hn, dn = nets
    n, params = BIG, (2, EXPLORE, 2, 1, 50, 23, SEED)
    _, takes_ev, outs = ENTRIES[GUMBEL]
    at = torch.arange(n, device=DEV) % 130
    st, tm, mask = (torch.from_numpy(x).to(DEV)[at].contiguous() for x in roots)
    out = {k: torch.full((n,) + tail, fill, dtype=getattr(torch, np.dtype(dt).name), device=DEV) for k, dt, tail, fill in outs}
    ev = dn[0].struct()
    nat.check(nat.lib().gbl_tree_search_gumbel(nat.ptr(st), nat.ptr(tm), nat.ptr(mask), C.addressof(ev), *params, ENV_BASE, 7,
                                               *[nat.ptr(out[o[0]]) for o in outs], n, nat.current_stream(DEV)), "gbl_tree_search_gumbel")
    torch.cuda.synchronize()
    for lo, hi in ((0, 64), (n - 130, n)):
        exp = run(GUMBEL, "cpu", *cycled(roots, lo, hi), params + (ENV_BASE + lo, 7), hn[0])
        for k, v in exp.items():
            assert torch.equal(out[k][lo:hi], torch.from_numpy(v).to(DEV)), (lo, k)
    assert (out["gumbel"][-130:] != 0).any() and int((out["action"] == -7).sum()) == 0


def test_k_collect_gumbel_more_boards_than_workgroups(G, boards, nets):
    """The same for self-play, one ply: the first 64 and the last 130 cells of every trajectory array, and the boards' final state."""
    hn, dn = nets
    n, its, considered = BIG, (2, 2), (2, 2)
    ps, ts, total = strides(n, 1, "time")
    at = torch.arange(n, device=DEV) % 130
    st, tm, turn = (torch.from_numpy(x).to(DEV)[at].contiguous() for x in boards)
    done = torch.full((n,), 5, dtype=torch.int8, device=DEV)
    traj = {k: torch.full((total,) + tail, 99 if dt == np.uint8 else -7, dtype=getattr(torch, np.dtype(dt).name), device=DEV)
            for k, dt, tail in EVAL_NAMES}
    evs = [x.struct() for x in dn]
    kw = dict(noise=1, visit_offset=50, scale=23, X=EXPLORE, sample_plies=0, seed=SEED, ply0=3)
    nat.check(nat.lib().gbl_collect_search_gumbel(*call_args("gumbel", nat.ptr, st, tm, done, traj, n, ps, ts, SEED, ENV_BASE, 3, None, 1,
                                                             ("eval", "eval"), EXPLORE, 0, nat.ILLEGAL_NOOP, None, turn, nat.current_stream(DEV),
                                                             evs=evs, its=its, considered=considered, gumbel_noise=1, visit_offset=50, scale=23)),
              "gbl_collect_search_gumbel")
    torch.cuda.synchronize()
    for lo, hi in ((0, 64), (n - 130, n)):
        exp = host_collect_gumbel(*cycled(boards, lo, hi), 1, ("eval", "eval"), hn, its, considered, env_base=ENV_BASE + lo, **kw)
        for k, v in exp[0].items():  # (T = 1 and a tile stride of 64: board b's cell is b)
            assert torch.equal(traj[k][lo:hi], torch.from_numpy(v[0]).to(DEV)), (lo, k)
        for name, mine, ref in zip(("state", "to_move", "done", "turn"), (st, tm, done, turn), exp[1:]):
            assert torch.equal(mine[lo:hi], torch.from_numpy(ref).to(DEV)), (lo, name)
    for k, v in traj.items():  # nothing past the last board's cell is written
        assert bool((v[n:] == (99 if v.dtype == torch.uint8 else -7)).all()), k
    assert bool((traj["how"][:n] == nat.HOW_GUMBEL).all())
