"""gbl_collect_search_tb on the MI355X (-m gpu): k_collect_tb against the host flavour byte for byte, every output between canaries
(tests/selfplay_tb_harness.py), at the batch sizes around a tile's edge and over the policy grid of tests/test_selfplay_tb.py; the
full inventory on 1 423^3 pseudo-random bytes against the composed device loop gbl_tb_probe + gbl_step_into, where successor indices
lie on both sides of 2^31; NULL optional outputs; a batch beyond the grid cap; a collect right behind the last sweep on one stream; a
graph capture and replay with ply_dev; and BatchedGobblet.collect with a table side against the same on "cpu", judge() included."""
import numpy as np
import pytest
import torch

from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as ER
from tests import selfplay_tb_harness as H
from tests import tablebase_harness as TH
from tests import tb_targets_restatement as TR
from tests.search_harness import G  # noqa: F401  (the fixture)
from tests.selfplay_harness import DEV, DeviceNet, _evaluator, same
from tests.test_gpu_tb_targets import full_inventory_rows
from tests.test_selfplay_solve import smoke_net
from tests.test_selfplay_tb import DEEP, POLICIES, WINDOWS, X

pytestmark = pytest.mark.gpu

GRID_CAP = 1 << 20
T = 5


@pytest.fixture(scope="module")
def world(G):
    """The (2, 2, 0) table built on the device and copied to the host: (device Table, host Table, host flavour, G.Tablebase)."""
    tb = G.Tablebase(DEEP, DEV)
    tb.build()
    assert tb.complete
    host = TH.Host(DEEP)
    assert np.array_equal(tb._aux.cpu().numpy(), host.aux)
    return H.Table(DEEP, tb._aux, tb.table), H.Table(DEEP, host.aux, tb.table.cpu().numpy()), host, tb


@pytest.fixture(scope="module")
def pool(world):
    """257 start boards of the three kinds, mixed; board 0 is a position of the table at turn 0 (a sampled table ply)."""
    st, tm, turn = H.start_boards(world[2], 150, 80, 27, seed=71)
    order = np.concatenate([[0], 1 + np.random.default_rng(72).permutation(len(st) - 1)])
    turn[0] = 0
    return st[order], tm[order], turn[order]


@pytest.fixture(scope="module")
def nets(G):
    pair = (smoke_net(), ER.random_net(128, 77))
    return pair, tuple(DeviceNet(x) for x in pair)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257])
def test_kernel_equals_host_flavour(world, pool, nets, n):
    dev, hst, _, _ = world
    hn, dn = nets
    st, tm, turn = (x[:n] for x in pool)
    hows = set()
    for i, (pols, its, deps, noise, judge) in enumerate(POLICIES):
        keep = None if judge else [k for k, _, _ in H.SOLVE_NAMES]
        for layout, illegal_mode, sample_plies, mode, count, ply_dev in (WINDOWS[i % 4], WINDOWS[(i + 1) % 4]):
            args = (its, deps, noise, X, sample_plies, illegal_mode, layout, 9, (1 << 40) + 5, 9 - (ply_dev or 0), ply_dev, mode, count, keep)
            got = H.device_collect_tb(dev, st, tm, turn, T, pols, tuple(d if p == "eval" else None for d, p in zip(dn, pols)), *args)
            same(got, H.host_collect_tb(hst, st, tm, turn, T, pols, tuple(h if p == "eval" else None for h, p in zip(hn, pols)), *args))
            hows |= set(got[0]["how"].ravel().tolist())
    assert {nat.HOW_TABLE, nat.HOW_TABLE_SAMPLED, nat.HOW_RANDOM} <= hows
    if n >= 63:
        assert nat.HOW_SEARCH in hows


def test_full_inventory_offsets_beyond_2_to_the_31(G):
    """1 024 boards of masked-random play, 4 plies of table against table on 1 423^3 pseudo-random bytes (no build: the rule reads
    whatever bytes there are), against gbl_tb_probe + the restated row + gbl_step_into on the device, ply by ply."""
    obs, _, _, _ = full_inventory_rows(G, 1024, tuple(range(6, 17)))
    n, plies, count = len(obs), 4, 7
    L, stream = nat.lib(), nat.current_stream(DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(61)
    table = torch.randint(-128, 128, (TH.FULL_POSITIONS,), dtype=torch.int8, device=DEV, generator=gen)
    aux = torch.zeros(nat.TB_AUX_BYTES, dtype=torch.uint8, device=DEV)
    tab = H.Table(TH.FULL, aux, table)
    assert L.gbl_tb_prepare(tab.inv, aux.data_ptr(), stream) == 0
    st, tm = torch.empty((n, 27), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)
    assert L.gbl_decode_obs(torch.from_numpy(obs).to(DEV).data_ptr(), st.data_ptr(), tm.data_ptr(), n, stream) == 0
    st0, tm0 = st.cpu().numpy(), tm.cpu().numpy()
    assert set(tm0.tolist()) == {0, 1}
    got = H.device_collect_tb(tab, st0, tm0, None, plies, ("tb", "tb"), seed=3, mode=1, count=count)
    tr = got[0]
    # the composed loop, from the same boards
    dn = torch.zeros(n, dtype=torch.int8, device=DEV)
    host_full = TH.Host(TH.FULL)
    index = []
    for t in range(plies):
        out = {"outcome": torch.empty((n, 54), dtype=torch.int8, device=DEV), "value": torch.empty(n, dtype=torch.int8, device=DEV),
               "action": torch.empty(n, dtype=torch.int32, device=DEV)}
        assert L.gbl_tb_probe(tab.inv, aux.data_ptr(), table.data_ptr(), st.data_ptr(), tm.data_ptr(), None, out["outcome"].data_ptr(),
                              out["value"].data_ptr(), out["action"].data_ptr(), n, stream) == 0
        p = {k: v.cpu().numpy() for k, v in out.items()}
        assert (p["action"] >= 0).all()
        mover = tm.cpu().numpy().copy()
        step = {"winner": torch.empty(n, dtype=torch.int8, device=DEV), "rewards": torch.empty((n, 2), dtype=torch.int8, device=DEV),
                "action_mask": torch.empty((n, 54), dtype=torch.int8, device=DEV), "observation": torch.empty((n, 117), dtype=torch.int8, device=DEV)}
        assert L.gbl_step_into(st.data_ptr(), tm.data_ptr(), dn.data_ptr(), out["action"].data_ptr(), step["winner"].data_ptr(),
                               step["rewards"].data_ptr(), step["action_mask"].data_ptr(), step["observation"].data_ptr(), None, None, None,
                               None, n, nat.ILLEGAL_NOOP, 1, stream) == 0
        exp = TR.targets(p["outcome"], p["value"], p["action"], TR.SHORTEST, count)
        for k, v in (("actions", p["action"]), ("visits", exp["visits"]), ("tb_outcomes", p["outcome"]), ("tb_value", p["value"]),
                     ("tb_played", p["outcome"][np.arange(n), p["action"]]), ("mover", mover), ("done", dn.cpu().numpy()),
                     ("to_move", tm.cpu().numpy()), ("value", (np.sign(p["value"].astype(np.int64)) * 128 * exp["visits"].astype(np.int64).sum(1)).astype(np.int32)),
                     ("how", np.full(n, nat.HOW_TABLE, np.int8)), ("nodes", np.zeros(n, np.int32)), ("root_value", np.zeros(n, np.int32)),
                     ("priors", np.zeros((n, 54), np.uint8)), ("outcomes", np.full((n, 54), nat.SOLVE_NONE, np.int8)), ("proven", np.zeros(n, np.int8)),
                     *[(k, v.cpu().numpy()) for k, v in step.items()]):
            assert tr[k][t].dtype == v.dtype and np.array_equal(tr[k][t], v), (t, k)
        quiet = dn.cpu().numpy() == 0
        index.append(host_full.index(st.cpu().numpy()[quiet], tm.cpu().numpy()[quiet]))  # the successors the next ply's table reads lie around
    assert np.array_equal(got[1], st.cpu().numpy()) and np.array_equal(got[2], tm.cpu().numpy())
    index = np.concatenate(index)
    assert (index >= 0).all() and (index > 1 << 31).sum() > 10 and (index < 1 << 31).sum() > 10


def test_null_optional_outputs(world, pool, nets):
    dev = world[0]
    _, dn = nets
    st, tm, turn = (x[:130] for x in pool)
    args = dict(nets=(dn[0], None), its=(4, 0), deps=(2, 0), noise=(32, 0), sample_plies=2, seed=5, count=3)
    full = H.device_collect_tb(dev, st, tm, turn, 3, ("eval", "tb"), **args)
    for keep in (("actions",), ("tb_outcomes",), ("tb_value",), ("tb_played",), ("tb_played", "visits"), ("tb_outcomes", "tb_value", "outcomes"),
                 ("value", "nodes", "how", "mover", "observation", "proven"), ("action_mask", "priors", "root_value", "tb_value", "tb_played"), ()):
        got = H.device_collect_tb(dev, st, tm, turn, 3, ("eval", "tb"), keep=keep, **args)
        assert set(got[0]) == set(keep)
        same(got, ({k: full[0][k] for k in keep},) + full[1:])


def test_beyond_the_grid_cap(world):
    """2^20 + 65 boards, one ply: boards of the table only (a table ply depends on the board alone, so the batch repeats its head)."""
    dev, hst, host, _ = world
    hst_st, hst_tm = TH.sample_boards(host, 4096, seed=73)
    n = GRID_CAP + 65
    st, tm = np.resize(hst_st, (n, 27)), np.resize(hst_tm, n)
    keep = ("actions", "visits", "how", "tb_value", "tb_played")
    got = H.device_collect_tb(dev, st, tm, None, 1, ("tb", "tb"), layout="tile", seed=3, mode=1, count=2, keep=keep)
    head = H.host_collect_tb(hst, hst_st, hst_tm, None, 1, ("tb", "tb"), layout="tile", seed=3, mode=1, count=2, keep=keep)
    assert (head[0]["how"] == nat.HOW_TABLE).all()
    for k in keep:
        assert np.array_equal(got[0][k], head[0][k][:, np.arange(n) % 4096]), k
    assert np.array_equal(got[1], np.resize(head[1], (n, 27)))


def test_a_collect_behind_the_last_sweep_needs_no_synchronisation(G, world):
    """Every sweep of a second table and then the collect go out on one stream with nothing in between."""
    built = world[3]
    kw = dict(policies=("tablebase", "random"), search=dict(tb_mode="shortest", tb_count=3, judge=True, sample_plies=2))

    def env():
        e = G.BatchedGobblet(300, DEV, auto_reset=True, seed=13, track_turn=True)
        return e
    ref = env().collect(6, out="fresh", **{**kw, "search": dict(kw["search"], tablebase=built)})
    torch.cuda.synchronize()
    e2 = env()
    with torch.cuda.stream(torch.cuda.Stream(DEV)):
        tb = G.Tablebase(DEEP, DEV)
        for k in range(built.sweeps):
            tb.sweep(k)
        out = e2.collect(6, out="fresh", **{**kw, "search": dict(kw["search"], tablebase=tb, allow_incomplete=True)})
        torch.cuda.current_stream().synchronize()
    assert torch.equal(tb.table, built.table)
    for k in ("actions", "visits", "how", "tb_outcomes", "tb_value", "tb_played", "observation"):
        assert torch.equal(out[k], ref[k]), k
    assert (out["how"] == nat.HOW_TABLE).any()


KEYS = ("actions", "visits", "value", "nodes", "how", "mover", "tb_outcomes", "tb_value", "tb_played", "observation", "done")


def test_graph_capture_and_replay(G, world):
    """One captured launch with ply_dev, replayed twice (gbl_counter_add advances the ply inside the graph): two eager launches."""
    n, T_, seed = 300, 3, 7
    kw = dict(policies=("tablebase", "random"), search=dict(tablebase=world[3], judge=True, sample_plies=2, tb_count=5))
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
    assert (seen[0]["how"] == nat.HOW_TABLE_SAMPLED).any() and (seen[1]["how"] == nat.HOW_RANDOM).any()
    assert not torch.equal(seen[0]["actions"], seen[1]["actions"])


def test_collect_with_a_table_side_equals_cpu(G, world):
    net = smoke_net()
    outs = []
    for d in (DEV, "cpu"):
        tb = world[3]
        if d == "cpu":
            tb = G.Tablebase(DEEP, "cpu")
            tb.table.copy_(world[3].table.cpu())
            tb.sweeps, tb.complete = world[3].sweeps, True
        env = G.BatchedGobblet(200, d, auto_reset=True, seed=11, env_base=3, track_turn=True)
        env.rollout(2)
        out = env.collect(6, policies=("evaluator", "tablebase"), count=True,
                          search=dict(evaluator=_evaluator(net, d), iterations=8, solve_depth=2, noise=0.25, sample_plies=4, explore=24,
                                      tablebase=tb, tb_mode="result", tb_count=4, judge=True))
        env.outcome_targets(out)
        outs.append((out, env, tb.judge(out)))
    torch.cuda.synchronize()
    (a, ea, ca), (b, eb, cb) = outs
    for k in KEYS + ("z", "plies_left", "action_mask", "winner", "rewards", "to_move", "root_value", "priors", "outcomes", "proven", "z_exact",
                     "regret"):
        assert torch.equal(a[k].cpu(), b[k]), k
    assert ca == cb and sum(sum(v.values()) for v in ca.values()) == 6 * 200
    assert torch.equal(ea.squares.cpu(), eb.squares) and torch.equal(ea.turn.cpu(), eb.turn) and int(ea.counters[0]) == 1200
    hows = set(a["how"].cpu().numpy().ravel().tolist())
    assert {nat.HOW_TABLE, nat.HOW_RANDOM} <= hows and (nat.HOW_SEARCH in hows or nat.HOW_SEARCH_SAMPLED in hows)
