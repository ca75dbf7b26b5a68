"""ReplayBuffer.relabel and fit(..., targets=) on the host flavour (no GPU): the relabelled ring against Tablebase.targets applied to the
ring's unpadded views (tests/test_tb_targets.py holds that to the rule), with the mover bytes, the tags, the padding and the slots
never written unchanged; a fit on exact targets against the hand-written loop of draw, targets, step, bit for bit; targets=None
against the loop without it.  The table is the complete (2, 2, 0) one: rows of the tree search's full-inventory self-play that hold a
large piece are no state of it and come out unlabelled."""
import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import symmetry_restatement as S


@pytest.fixture(scope="module")
def tb():
    t = G.Tablebase((2, 2, 0), "cpu")
    t.build()
    assert t.complete
    return t


@pytest.fixture(scope="module")
def window():
    env = G.BatchedGobblet(130, "cpu", auto_reset=True, seed=5, track_turn=True)
    traj = env.collect(6, policies=("tree", "tree"), search=S.SEARCH)
    env.outcome_targets(traj)
    return env, traj


def views(buf, rows):
    return {"observation": buf.observation[:rows].clone(), "action_mask": buf.action_mask[:rows].clone(), "visits": buf.visits[:rows].clone(),
            "z": buf.z[:rows].clone()}


@pytest.mark.parametrize("capacity, appends", [(300, 1), (150, 2)])
@pytest.mark.parametrize("mode, count", [("result", 1), ("shortest", 600)])
def test_relabel_equals_targets_on_the_unpadded_views(tb, window, capacity, appends, mode, count):
    env, traj = window
    buf = G.ReplayBuffer(capacity, "cpu")
    for g in range(appends):
        buf.append(env, traj, tag=7 + g)
    live = buf.size
    assert (live < capacity) == (appends == 1) and live > 75
    obs, visits, meta = buf._obs.clone(), buf._visits.clone(), buf._meta.clone()
    exp = tb.targets(views(buf, live), mode=mode, count=count, census=True)
    census = buf.relabel(tb, mode=mode, count=count, census=True)
    assert buf.relabel(tb, mode=mode, count=count) is None                          # (the exact targets are a fixed point ...)
    assert torch.equal(buf.visits[:live], exp["visits"]) and torch.equal(buf.z[:live], exp["z"]) and torch.equal(census, exp["census"])
    assert census.shape == (live,) and (census >= 0).sum() > 20 and (census < 0).sum() > 20
    assert int(buf.visits[:live].max()) == count and set(buf.z[:live][census >= 0].tolist()) <= {-1, 0, 1}
    assert (buf.z[:live][census < 0] == nat.Z_OPEN).all() and not buf.visits[:live][census < 0].any()
    # observations, masks, mover bytes, tags and every padding byte as they were; a slot never written stays zero
    keep = torch.ones(nat.REPLAY_META_PITCH, dtype=torch.bool)
    keep[nat.REPLAY_META_Z] = False
    assert torch.equal(buf._obs, obs) and torch.equal(buf._meta[:, keep], meta[:, keep]) and torch.equal(buf._visits[:, nat.ACTIONS:], visits[:, nat.ACTIONS:])
    assert not buf._obs[live:].any() and not buf._visits[live:].any() and not buf._meta[live:].any()
    again = tb.targets(views(buf, live), mode=mode, count=count, census=True)      # (... whose census says so: every argmax in R, every z right)
    assert ((again["census"] & 3) == 3)[again["census"] >= 0].all()


def test_relabel_and_targets_refuse_what_they_cannot_label(tb, window):
    env, traj = window
    bare = G.ReplayBuffer(150, "cpu", observations=False)
    bare.append(env, traj)
    with pytest.raises(ValueError, match="observations"):
        bare.relabel(tb)
    buf = G.ReplayBuffer(150, "cpu")
    buf.append(env, traj)
    young = G.Tablebase((1, 1, 0), "cpu")
    with pytest.raises(ValueError, match="not complete"):
        buf.relabel(young)
    assert buf.relabel(young, allow_incomplete=True, census=True).shape == (buf.size,)
    young.device = torch.device("meta")
    with pytest.raises(ValueError, match="lives on"):
        buf.relabel(young, allow_incomplete=True)
    with pytest.raises(ValueError, match="on cpu"):
        tb.targets({k: v.to("meta") for k, v in views(buf, 8).items()})
    empty = G.ReplayBuffer(16, "cpu")
    assert empty.relabel(tb, census=True).shape == (0,) and not empty._meta.any()


def test_fit_on_exact_targets_equals_the_hand_written_loop(tb, window):
    env, traj = window
    buf = G.ReplayBuffer(200, "cpu")
    buf.append(env, traj, tag=1)
    buf.append(env, traj, tag=2)
    a, b, c, d = (G.GobbletTrainer(hidden=64, device="cpu", seed=1) for _ in range(4))
    stats = buf.fit(a, 3, batch=256, symmetries="all", first_call=7, recent=100, targets=tb)
    by_hand = torch.stack([b.step(tb.targets(buf.batch(256, symmetries="all", call=7 + i, recent=100))) for i in range(3)])
    assert torch.equal(stats, by_hand) and torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert 0 < float(stats[:, 2].min()) < 256                                       # (the unlabelled rows count for nothing)
    # targets=None is the loop as it was: draw, step
    plain = buf.fit(c, 3, batch=256, symmetries="all", first_call=7, recent=100)
    before = torch.stack([d.step(buf.batch(256, symmetries="all", call=7 + i, recent=100)) for i in range(3)])
    assert torch.equal(plain, before) and torch.equal(c.params, d.params) and float(plain[:, 2].min()) == 256
    assert not torch.equal(a.params, c.params)
    # the environment's fit likewise, on the window itself
    e, f = G.GobbletTrainer(hidden=64, device="cpu", seed=2), G.GobbletTrainer(hidden=64, device="cpu", seed=2)
    stats = env.fit(traj, e, 3, batch=128, first_call=2, targets=tb)
    by_hand = torch.stack([f.step(tb.targets(env.training_batch(traj, 128, call=2 + i))) for i in range(3)])
    assert torch.equal(stats, by_hand) and torch.equal(e.params, f.params)


def test_the_tablebase_training_example_runs_on_the_host_flavour():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_train_tablebase", os.path.join(root, "examples", "example_train_tablebase.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.train_both("cpu", inventory=(2, 2, 0), windows=2, boards=128, plies=12, steps=3, batch=128, iterations=8, capacity=2048, held_out=256)
    assert set(out) == {"search", "exact"} and out["search"]["rows"] == out["exact"]["rows"] > 0
    assert all(0.0 <= r[k] <= 1.0 for r in out.values() for k in ("value_sign", "top_prior_in_R"))
