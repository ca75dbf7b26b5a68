"""gbl_cpu_reanalyse (include/gobblet_hip.h, "Reanalysis") against the restatement of its rule (tests/reanalyse_restatement.py: the decode,
restate_search and the header's sentences in Python integers), byte for byte through guard bytes; the fixed point on a self-play ring;
the recorded argument errors on both flavours; and the Python surface on the host flavour.  No GPU.  Rows: the live rows of a 64-board,
12-ply evaluator self-play ring (H = 64, a seeded random_net) and 32 masked-random positions."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import reanalyse_harness as H
from tests import reanalyse_restatement as RR
from tests.search_harness import replay_arg_errors
from tests.tb_targets_harness import BATCH, RING

EXPLORE = H.EXPLORE


@pytest.fixture(scope="module")
def world():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    net = H.net64()
    rows = H.make_rows(net)
    assert len(rows[0]) > 200 and (rows[3] == nat.Z_OPEN).sum() >= 3
    yield H.Env(net), rows, {}
    L.gbl_cpu_set_threads(0)


def searched(world, iterations, masked):
    """The restatement's search of every row, computed once per (iterations, mask given) and left unchanged."""
    env, (obs, mask, _, _), cache = world
    if (iterations, masked) not in cache:
        cache[iterations, masked] = RR.searched(env.net, obs, mask if masked else None, iterations, EXPLORE)
    return cache[iterations, masked]


def expected(world, iterations, masked, v_old, z_old, pick=slice(None)):
    s = {k: v[pick] for k, v in searched(world, iterations, masked).items()}
    return RR.reanalyse(s, None if v_old is None else v_old[pick], None if z_old is None else z_old[pick])


def case(world, iterations, masked, what, with_visits=True, with_z=True, pick=slice(None), **kw):
    env, (obs, mask, v_old, z_old), _ = world
    v, z = (v_old if with_visits else None), (z_old if with_z else None)
    exp = expected(world, iterations, masked, v, z, pick)
    got = H.run(env, obs[pick], mask[pick] if masked else None, None if v is None else v[pick], None if z is None else z[pick], iterations, **kw)
    inplace = kw.get("inplace", True) and with_visits
    H.check(got, exp, v_old[pick] if inplace else 0x5A5A, what)
    return got, exp


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("iterations", [1, 8, 64])
def test_host_flavour_equals_the_restatement(world, iterations, masked):
    seen = set()
    for layout in (BATCH, RING):
        for inplace in (True, False):
            got, exp = case(world, iterations, masked, (layout is RING, inplace), layout=layout, inplace=inplace, lead=1)
            seen |= set(exp["census"].tolist())
    live = exp["census"] >= 0
    assert (~exp["written"]).sum() >= 3 and live.sum() > 200
    assert (got["visits"][live].sum(1) == iterations).all() and (exp["nodes"][live] >= 2).all() and (exp["drift"][live] >= 0).all()
    assert {-1, 0, 1, 2, 3} <= seen


@pytest.mark.parametrize("masked", [True, False])
def test_every_dense_output_on_its_own_and_every_optional_input(world, masked):
    for keep in [(k,) for k in H.ALL] + [()]:
        case(world, 8, masked, keep, keep=keep, lead=3)
        case(world, 8, masked, keep, keep=keep, layout=RING, inplace=False)
    got, exp = case(world, 8, masked, "no visits_in", with_visits=False)
    live = exp["census"] >= 0
    assert (exp["drift"] == -1).all() and ((exp["census"][live] & 4) != 0).all()
    got, exp = case(world, 8, masked, "no z_in", with_z=False)
    assert exp["written"].all() and not (exp["census"] & 2).any()
    case(world, 8, masked, "no optional input", with_visits=False, with_z=False, layout=RING)
    # visits_out NULL: the dense outputs as before, no visits row written
    env, (obs, mask, v_old, z_old), _ = world
    got = H.run(env, obs, mask if masked else None, v_old, z_old, 8, inplace=False, give_visits_out=False)
    exp = expected(world, 8, masked, v_old, z_old)
    assert all(np.array_equal(got[k], exp[k]) for k in H.ALL)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts(world, n):
    pick = np.arange(n) * 7 % len(world[1][0])
    for layout in (BATCH, RING):
        case(world, 8, True, n, pick=pick, layout=layout)


def test_in_place_equals_separate_outputs(world):
    env, (obs, mask, v_old, z_old), _ = world
    z = np.where(z_old == nat.Z_OPEN, 0, z_old).astype(np.int8)          # (no skipped row: every output byte is defined)
    a = H.run(env, obs, mask, v_old, z, 8, inplace=True, layout=RING)
    b = H.run(env, obs, mask, v_old, z, 8, inplace=False, layout=RING)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_planted_rows(world):
    env, (obs, mask, v_old, z_old), _ = world
    base = np.flatnonzero((z_old != nat.Z_OPEN) & (mask != 0).any(1))[:8]
    p_obs, p_mask, p_v, p_z = obs[base].copy(), mask[base].copy(), v_old[base].copy(), z_old[base].copy()
    p_z[0] = nat.Z_OPEN                                                 # skipped
    p_mask[1] = 0                                                       # no candidate
    p_obs[2], p_mask[2] = 0, 1                                          # the empty board, player_1 to move
    p_v[3] = 0                                                          # no old visits
    p_v[4] = -5                                                         # ... or only negative ones
    p_v[5] = 32767                                                      # the drift's operand bound: So = 54 * 32767
    p_v[6] = 0
    p_v[6, np.flatnonzero(p_mask[6])[0]] = 32767                        # one old action
    for its in (1, 64, 512):
        s = RR.searched(env.net, p_obs, p_mask, its, EXPLORE)
        exp = RR.reanalyse(s, p_v, p_z)
        for layout in (BATCH, RING):
            for inplace in (True, False):
                got = H.run(env, p_obs, p_mask, p_v, p_z, its, layout=layout, inplace=inplace, lead=1)
                H.check(got, exp, p_v if inplace else 0x5A5A, (its, layout is RING, inplace))
        assert (got["root_value"][0], got["action"][0], got["nodes"][0], got["drift"][0], got["census"][0]) == (0, -1, 0, -1, -1)
        assert not got["root_priors"][0].any()
        assert not got["visits"][1].any() and (got["action"][1], got["nodes"][1], got["drift"][1], got["census"][1]) == (-1, 1, -1, -1)
        assert got["root_value"][1] == s["root_value"][1] and not got["root_priors"][1].any()
        assert not s["state"][2].any() and s["to_move"][2] == 0 and got["visits"][2].sum() == its and (got["root_priors"][2] > 0).all()
        assert got["drift"][3] == got["drift"][4] == 1024 and (got["census"][3] & 4) and (got["census"][4] & 4) and not (got["census"][3] & 1)
        assert 0 <= got["drift"][5] <= 1024 and not (got["census"][5] & 4)
        assert 0 <= got["drift"][6] <= 1024


def test_a_legal_interleave_of_an_output_with_an_input(world):
    """visits_out's rows inside the gaps of obs's rows, both 256 bytes apart: every byte distinct, so the call is legal and right."""
    env, (obs, mask, v_old, z_old), _ = world
    n = 40
    raw = np.full(256 * n + 64, 0x5A, np.uint8)
    raw = raw[-raw.ctypes.data % 64:]
    for r in range(n):
        raw[256 * r:256 * r + 117] = obs[r].view(np.uint8)
    before = raw.copy()
    ev = env.net.struct()
    rc = env.L.gbl_cpu_reanalyse(C.addressof(ev), 8, EXPLORE, raw.ctypes.data, 256, None, 54, None, raw.ctypes.data + 118, 128, None, 1,
                                 None, None, None, None, None, None, n, None)
    assert rc == 0, env.error()
    exp = expected(world, 8, False, None, None, slice(0, n))
    rows = np.stack([raw[256 * r + 118:256 * r + 226].view(np.int16) for r in range(n)])
    assert np.array_equal(rows, exp["visits"])
    written = np.zeros(len(raw), bool)
    for r in range(n):
        written[256 * r + 118:256 * r + 226] = True
    assert np.array_equal(raw[~written], before[~written])


# ---- the ring: the fixed point, the doubling check, the untouched bytes -----------------------------------------------------------------
def ring_bytes(buf):
    return buf._obs.clone(), buf._visits.clone(), buf._meta.clone()


def check_fixed_point_and_untouched_bytes(device):
    net = H.net64()
    buf, ev = H.selfplay_ring(net, device, iterations=8, sample_plies=4, capacity=600)
    live = buf.size
    assert 100 < live < 600
    before = ring_bytes(buf)
    out = buf.reanalyse(ev, iterations=8, explore=EXPLORE, census=True)
    for a, b in zip(ring_bytes(buf), before):
        assert torch.equal(a, b)                                       # the stored visits ARE this search's
    assert out["drift"].shape == out["census"].shape == (live,)
    assert (out["drift"] == 0).all() and ((out["census"] & 1) == 1).all()
    # twice the iterations: some row changes, every row's visits sum to the iterations, and nothing else moves
    out = buf.reanalyse(ev, iterations=16, explore=EXPLORE)
    assert out["census"] is None
    obs, visits, meta = ring_bytes(buf)
    assert torch.equal(obs, before[0]) and torch.equal(meta, before[2])
    assert torch.equal(visits[:, nat.ACTIONS:], before[1][:, nat.ACTIONS:]) and torch.equal(visits[live:], before[1][live:])
    assert not torch.equal(visits[:live], before[1][:live]) and (visits[:live, :nat.ACTIONS].to(torch.int32).sum(1) == 16).all()
    assert (out["drift"] >= 0).all() and (out["drift"] > 0).any()
    return buf, ev, out


def test_fixed_point_doubling_and_untouched_ring_bytes():
    check_fixed_point_and_untouched_bytes("cpu")


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_replay_the_recorded_table(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "reanalyse_arg_errors.json")))
    assert len(table) > 40 and {c["fn"] for c in table} == {"reanalyse"}
    replay_arg_errors(table)
    both = [c for c in table if c["host"] is not None]
    assert all(c["host"][0] == c["device"][0] for c in both)            # the same codes on both flavours
    assert sum(c["host"] is None and c["device"][0] == nat.ERR_ALIGN for c in table) >= 8
    # the stated order: each case that breaks two rules reports the earlier one
    order = [c["device"][1] for c in table if c["case"].startswith("order:")]
    assert len(order) >= 8


# ---- the Python surface on the host flavour ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring(world):
    env = world[0]
    buf, ev = H.selfplay_ring(env.net, "cpu", iterations=8, sample_plies=4, capacity=600, prioritized=True)
    return buf, ev


def test_evaluator_reanalyse_on_a_batch_dict(world, ring):
    env = world[0]
    buf, ev = ring
    batch = buf.batch(96, symmetries=None, call=3, seed=1)
    before = {k: v.clone() for k, v in batch.items()}
    out = ev.reanalyse(batch, iterations=16, explore=EXPLORE, census=True)
    assert all(torch.equal(batch[k], before[k]) for k in before) and out["visits"] is not batch["visits"]      # not in place
    assert set(out) == set(batch) | {"root_value", "drift", "census"} and all(out[k] is batch[k] for k in batch if k != "visits")
    s = RR.searched(env.net, before["observation"].numpy(), before["action_mask"].numpy(), 16, EXPLORE)
    exp = RR.reanalyse(s, before["visits"].numpy(), before["z"].numpy())
    H.check({k: out[k].numpy() for k in ("visits", "root_value", "drift", "census")}, exp, before["visits"].numpy())
    assert "census" not in ev.reanalyse(batch, iterations=16)
    visits = batch["visits"]
    same = ev.reanalyse(batch, iterations=16, explore=EXPLORE, out=visits)                                        # the in-place form
    assert same["visits"] is visits and torch.equal(visits, out["visits"])
    for bad, why in (({k: v for k, v in batch.items() if k != "observation"}, "observation"), (dict(batch, z=batch["z"].to(torch.int16)), "z must be")):
        with pytest.raises(ValueError, match=why):
            ev.reanalyse(bad)
    with pytest.raises(ValueError, match="iterations"):
        ev.reanalyse(batch, iterations=513)
    with pytest.raises(ValueError, match="out must be"):
        ev.reanalyse(batch, out=torch.zeros((96, 54), dtype=torch.int32))


def test_ring_reanalyse_sets_priorities_from_the_drift(world, ring):
    buf, ev = ring
    state = buf.state_dict()
    live = buf.size
    plain = buf.reanalyse(ev, iterations=16, explore=EXPLORE)
    assert (buf.priority[:live] == 1).all()                                                                    # (append's default, untouched)
    buf.load_state_dict(state)
    out = buf.reanalyse(ev, iterations=16, explore=EXPLORE, census=True, prioritize=dict(floor=3, scale=5))
    assert torch.equal(out["drift"], plain["drift"]) and (out["drift"] > 0).any()
    assert torch.equal(buf.priority[:live], (3 + 5 * out["drift"].clamp(min=0)).to(torch.int32)) and not buf.priority[live:].any()
    drawn = buf.batch(64, call=1, prioritized=True)
    assert (drawn["index"][:, 0] >= 0).all()
    plainbuf = G.ReplayBuffer(16, "cpu")
    with pytest.raises(ValueError, match="prioritized=True"):
        plainbuf.reanalyse(ev, prioritize=dict(floor=1))
    with pytest.raises(ValueError, match="observations"):
        G.ReplayBuffer(16, "cpu", observations=False).reanalyse(ev)
    empty = plainbuf.reanalyse(ev, census=True)
    assert empty["drift"].shape == empty["census"].shape == (0,) and not plainbuf._visits.any()
    buf.load_state_dict(state)


def test_fit_with_reanalyse_equals_the_hand_written_loop(world, ring):
    buf, ev = ring
    tb = G.Tablebase((1, 1, 0), "cpu")
    spec = dict(evaluator=ev, iterations=8, explore=EXPLORE)
    a, b, c, d, e = (G.GobbletTrainer(hidden=64, device="cpu", seed=1) for _ in range(5))
    stats = buf.fit(a, 3, batch=128, symmetries="all", first_call=5, recent=150, reanalyse=spec)
    by_hand = torch.stack([b.step(ev.reanalyse(buf.batch(128, symmetries="all", call=5 + i, recent=150), 8, EXPLORE)) for i in range(3)])
    assert torch.equal(stats, by_hand) and torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    # more iterations than the stored rows' search had: the targets, and so the fit, differ from the plain one
    buf.fit(c, 3, batch=128, symmetries="all", first_call=5, recent=150, reanalyse=dict(spec, iterations=32))
    buf.fit(d, 3, batch=128, symmetries="all", first_call=5, recent=150)
    assert not torch.equal(c.params, d.params)
    # it composes with the prioritised loop
    hyper = dict(prioritized=True, beta=(0.4, 1.0), priority=dict(scale=64.0, floor=1, cap=1 << 20))
    state = buf.state_dict()
    stats = buf.fit(e, 3, batch=128, first_call=9, reanalyse=spec, **hyper)
    assert stats.shape == (3, 4) and torch.isfinite(stats).all()
    buf.load_state_dict(state)
    with pytest.raises(ValueError, match="exclude"):
        buf.fit(a, 1, targets=tb, reanalyse=spec)
    with pytest.raises(ValueError, match="reanalyse=dict"):
        buf.fit(a, 1, reanalyse=dict(iterations=8))


def test_the_reanalysis_example_runs_on_the_host_flavour():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_reanalyse", os.path.join(root, "examples", "example_reanalyse.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.train_both("cpu", inventory=(2, 2, 0), boards=128, plies=12, steps=3, batch=128, iterations=8, capacity=2048, held_out=256)
    assert set(out) == {"stale", "reanalysed"} and out["stale"]["rows"] == out["reanalysed"]["rows"] > 0
    assert all(0.0 <= r[k] <= 1.0 for r in out.values() for k in ("value_sign", "top_prior_in_R"))
    assert 0.0 <= out["reanalysed"]["mean_drift"] <= 1.0
