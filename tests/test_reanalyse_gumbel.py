"""gbl_cpu_reanalyse_gumbel (include/gobblet_hip.h, "Reanalysis with the Gumbel root rule") against the restatement of its rule
(tests/reanalyse_gumbel_restatement.py), byte for byte through guard bytes; against gbl_cpu_decode_obs + gbl_cpu_tree_search_gumbel, which
does not rest on the restatement; the identity on a Gumbel self-play ring; the drift's edges in exact integers; gbl_cpu_reanalyse
unchanged; the argument errors in their stated order on both flavours; and the Python surface on the host flavour.  No GPU.

The drift's 64-bit sum: the header bounds Sn by the bytes' range, 54 * 255, where 2 So Sn passes 2^32.  The target rule itself writes
bytes that sum to at most |C| + 254 <= 308 (a flat row over 54 candidates is 54 fives: 270), so no row an entry point produces reaches
that: the largest operands there are -- So = 54 * 32767 against a full row -- give 2 So Sn of about 1.1e9.  The edges below are
therefore the largest reachable ones, each compared with Python's integers."""
import ctypes as C

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as ER
from tests import reanalyse_gumbel_harness as GH
from tests import reanalyse_gumbel_restatement as GRR
from tests import reanalyse_harness as H
from tests import reanalyse_restatement as RR
from tests.tb_targets_harness import BATCH, RING

EXPLORE = GH.EXPLORE
SEED, ENV_BASE, CALL = 0x123456789ABCDEF, (1 << 33) + 5, 77
PAIRS = [(1, 8), (3, 8), (16, 16), (16, 64), (54, 16)]                 # (considered, iterations)
NOISE_SCALE = [(0, 23), (1, 23), (0, 0), (1, 0)]


@pytest.fixture(scope="module")
def world():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    nets = {64: H.net64(), 128: ER.random_net(128, 133)}
    rows = GH.planted_rows()
    yield {h: H.Env(n) for h, n in nets.items()}, rows
    L.gbl_cpu_set_threads(0)


def restated(env, rows, iterations, rule, masked=True, with_visits=True, with_z=True, keys=(SEED, ENV_BASE, CALL)):
    obs, mask, v_old, z_old = rows
    s = GRR.searched(env.net, obs, mask if masked else None, iterations, EXPLORE, *rule, *keys)
    return GRR.reanalyse(s, v_old if with_visits else None, z_old if with_z else None)


@pytest.mark.parametrize("noise,scale", NOISE_SCALE)
@pytest.mark.parametrize("considered,iterations", PAIRS)
@pytest.mark.parametrize("hidden", [64, 128])
def test_host_flavour_equals_the_restatement(world, hidden, considered, iterations, noise, scale):
    envs, rows = world
    env, rule = envs[hidden], (considered, noise, 50, scale)
    obs, mask, v_old, z_old = rows
    exp = restated(env, rows, iterations, rule)
    for layout, inplace, lead in ((BATCH, False, 1), (RING, True, 0), (BATCH, True, 3)):
        got = GH.run(env, obs, mask, v_old, z_old, iterations, rule, SEED, ENV_BASE, CALL, layout=layout, inplace=inplace, lead=lead)
        GH.check(got, exp, v_old if inplace else 0x5A5A, (layout is RING, inplace))
    live = exp["census"] >= 0
    cands = (exp["visits"] > 0).sum(1)
    assert (~exp["written"]).sum() == 3 and live.sum() == 16 and {54, 27, 3, 2, 1} <= set(cands[live].tolist())
    assert (exp["visits"][live].max(1) <= 255).all() and (exp["visits"][live].sum(1) <= cands[live] + 254).all()
    assert (exp["gumbel"] != 0).any() == bool(noise) and (exp["nodes"][live] >= 2).all()
    assert (exp["drift"][live] >= 0).all() and (exp["drift"][live] <= 1024).all()


def test_every_dense_output_on_its_own_and_every_optional_input(world):
    envs, rows = world
    env, rule = envs[64], GH.RULE
    obs, mask, v_old, z_old = rows
    exp = restated(env, rows, 16, rule)
    for keep in [(k,) for k in GH.ALL] + [()]:
        GH.check(GH.run(env, obs, mask, v_old, z_old, 16, rule, SEED, ENV_BASE, CALL, keep=keep, lead=3), exp, v_old, keep)
        GH.check(GH.run(env, obs, mask, v_old, z_old, 16, rule, SEED, ENV_BASE, CALL, keep=keep, layout=RING, inplace=False), exp, 0x5A5A, keep)
    e = restated(env, rows, 16, rule, with_visits=False)
    GH.check(GH.run(env, obs, mask, None, z_old, 16, rule, SEED, ENV_BASE, CALL), e, 0x5A5A, "no visits_in")
    assert (e["drift"] == -1).all() and ((e["census"][e["census"] >= 0] & 4) != 0).all()
    e = restated(env, rows, 16, rule, with_z=False)
    GH.check(GH.run(env, obs, mask, v_old, None, 16, rule, SEED, ENV_BASE, CALL), e, v_old, "no z_in")
    assert e["written"].all() and not (e["census"][e["census"] >= 0] & 2).any()
    e = restated(env, rows, 16, rule, masked=False, with_visits=False, with_z=False)
    GH.check(GH.run(env, obs, None, None, None, 16, rule, SEED, ENV_BASE, CALL, layout=RING), e, 0x5A5A, "no optional input")
    got = GH.run(env, obs, mask, v_old, z_old, 16, rule, SEED, ENV_BASE, CALL, inplace=False, give_visits_out=False)
    assert all(np.array_equal(got[k], exp[k]) for k in GH.ALL)


def test_noise_is_keyed_by_seed_row_and_call(world):
    envs, rows = world
    env = envs[64]
    obs, mask, v_old, _ = rows
    base = GH.run(env, obs, mask, v_old, None, 16, GH.RULE, SEED, ENV_BASE, CALL, inplace=False)
    again = GH.run(env, obs, mask, v_old, None, 16, GH.RULE, SEED, ENV_BASE, CALL, inplace=False)
    assert all(base[k].tobytes() == again[k].tobytes() for k in base)
    for keys in ((SEED + 1, ENV_BASE, CALL), (SEED, ENV_BASE + 1, CALL), (SEED, ENV_BASE, CALL + 1)):
        other = GH.run(env, obs, mask, v_old, None, 16, GH.RULE, *keys, inplace=False)
        assert not np.array_equal(other["gumbel"], base["gumbel"]), keys
    # row r of a call at env_base + 1 is board env_base + 1 + r: the noise of the rows shifts with the row index
    tail = GH.run(env, obs[1:], mask[1:], v_old[1:], None, 16, GH.RULE, SEED, ENV_BASE + 1, CALL, inplace=False)
    assert all(tail[k].tobytes() == base[k][1:].tobytes() for k in base)
    # without noise nothing is drawn: the keys do not matter
    quiet = [GH.run(env, obs, mask, v_old, None, 16, (16, 0, 50, 23), *keys, inplace=False) for keys in ((0, 0, 0), (SEED, ENV_BASE, CALL))]
    assert all(quiet[0][k].tobytes() == quiet[1][k].tobytes() for k in quiet[0]) and not quiet[0]["gumbel"].any()


@pytest.mark.parametrize("considered,iterations,noise", [(16, 16, 1), (3, 8, 0), (54, 64, 1)])
def test_equals_decode_and_the_gumbel_search(world, considered, iterations, noise):
    """Not through the restatement: gbl_cpu_decode_obs, then gbl_cpu_tree_search_gumbel under the rows' masks with the same keys."""
    envs, rows = world
    env = envs[64]
    obs, mask, v_old, _ = rows
    n = len(obs)
    got = GH.run(env, obs, mask, v_old, None, iterations, (considered, noise, 50, 23), SEED, ENV_BASE, CALL, inplace=False)
    st, tm = RR.decode(obs)
    out = {k: np.zeros((n, 54) if k in ("visits", "wins", "losses") else n, np.int32) for k in ("visits", "wins", "losses", "action", "nodes", "root_value")}
    priors, target, gum = np.zeros((n, 54), np.uint8), np.zeros((n, 54), np.uint8), np.zeros((n, 54), np.int16)
    ev = env.net.struct()
    m = np.ascontiguousarray(mask)
    rc = env.L.gbl_cpu_tree_search_gumbel(st.ctypes.data, tm.ctypes.data, m.ctypes.data, C.addressof(ev), iterations, EXPLORE, considered, noise, 50,
                                          23, SEED, ENV_BASE, CALL, *[out[k].ctypes.data for k in out], priors.ctypes.data, target.ctypes.data,
                                          gum.ctypes.data, n, None)
    assert rc == 0, env.error()
    assert np.array_equal(got["visits"], target.astype(np.int16)) and (target > 0).any()
    for k in ("action", "nodes", "root_value"):
        assert np.array_equal(got[k], out[k]), k
    assert np.array_equal(got["root_priors"], priors) and np.array_equal(got["gumbel"], gum)


# ---- the identity on a ring of target rows ------------------------------------------------------------------------------------------
def ring_bytes(buf):
    return buf._obs.clone(), buf._visits.clone(), buf._meta.clone()


def check_identity_and_untouched_bytes(device):
    rule = (16, 0, 50, 23)
    spec = dict(considered=16, noise=False, visit_offset=50, scale=23)
    buf, ev = GH.gumbel_ring(H.net64(), device, rule=rule)
    live = buf.size
    assert 100 < live < 512
    before = ring_bytes(buf)
    assert int(before[1][:live, :nat.ACTIONS].max()) <= 255 and (before[1][:live, :nat.ACTIONS] > 0).sum(1).min() >= 1   # target rows
    out = buf.reanalyse(ev, iterations=16, explore=EXPLORE, census=True, gumbel=spec)
    for a, b in zip(ring_bytes(buf), before):
        assert torch.equal(a, b)                                       # the stored rows ARE this search's target rows
    assert out["drift"].shape == out["census"].shape == (live,)
    assert (out["drift"] == 0).all() and ((out["census"] & 1) == 1).all()
    # with noise the target row has no g in it, but the schedule visits other actions: some row moves, and nothing else does
    out = buf.reanalyse(ev, iterations=16, explore=EXPLORE, gumbel=dict(spec, noise=True), seed=3, call=2)
    obs, visits, meta = ring_bytes(buf)
    assert torch.equal(obs, before[0]) and torch.equal(meta, before[2])
    assert torch.equal(visits[:, nat.ACTIONS:], before[1][:, nat.ACTIONS:]) and torch.equal(visits[live:], before[1][live:])
    assert not torch.equal(visits[:live], before[1][:live]) and (out["drift"] >= 0).all() and (out["drift"] > 0).any()
    return buf, ev, out


def test_identity_on_a_gumbel_ring_and_untouched_ring_bytes():
    check_identity_and_untouched_bytes("cpu")


# ---- the drift's edges, in Python's integers ----------------------------------------------------------------------------------------
def exact_drift(old, new):
    o, n = [max(int(x), 0) for x in old], [int(x) for x in new]
    so, sn = sum(o), sum(n)
    return 1024 if so == 0 else (1024 * sum(abs(a * sn - b * so) for a, b in zip(o, n))) // (2 * so * sn)


def drift_edge_rows():
    """The empty board (all 54 actions are candidates) under a network of zeros: a flat target row over 54 candidates.  Old rows: 32767 on five
    actions, 32767 on all 54 (So = 54 * 32767), negative entries among positive ones, only negative ones, zeros."""
    n = 5
    obs, mask = np.zeros((n, 117), np.int8), np.ones((n, 54), np.int8)
    v = np.zeros((n, 54), np.int16)
    v[0, [0, 1, 2, 30, 53]] = 32767
    v[1] = 32767
    v[2, :10], v[2, 10:20] = -7, 9
    v[3] = -1
    return obs, mask, v


def check_drift_edges(env_zero, env):
    obs, mask, v = drift_edge_rows()
    for e, flat in ((env_zero, True), (env, False)):
        got = GH.run(e, obs, mask, v, None, 16, (16, 0, 50, 23), inplace=False)
        new = got["visits"]
        assert (new > 0).all() and (not flat or (new == 1 + 254 // 54).all())
        assert got["drift"].tolist() == [exact_drift(v[r], new[r]) for r in range(5)] and got["drift"][3] == got["drift"][4] == 1024
        assert 0 < got["drift"][0] <= 1024 and 0 <= got["drift"][1] <= 1024 and (not flat or got["drift"][1] == 0)   # (flat against flat)
        assert got["drift"][2] == exact_drift(np.where(v[2] < 0, 0, v[2]), new[2])          # negative old entries count as 0
        nul = GH.run(e, obs, mask, None, None, 16, (16, 0, 50, 23))
        assert (nul["drift"] == -1).all() and np.array_equal(nul["visits"], new)
    return got


def test_drift_edges(world):
    got = check_drift_edges(H.Env(ER.zero_net(64)), world[0][64])
    # what the sums reach here: So = 54 * 32767 against a full row
    so, sn = 54 * 32767, int(got["visits"][1].sum())
    assert sn <= 54 + 254 and 2 * so * sn < 1 << 32


# ---- gbl_cpu_reanalyse is what it was ------------------------------------------------------------------------------------------------
def test_the_visit_count_form_is_unchanged():
    env = H.Env(H.net64())
    obs, mask, v_old, z_old = H.make_rows(env.net)
    pick = np.arange(257) * 7 % len(obs)
    obs, mask, v_old, z_old = obs[pick], mask[pick], v_old[pick], z_old[pick]
    assert (z_old == nat.Z_OPEN).any()
    for iterations in (8, 64):
        exp = RR.reanalyse(RR.searched(env.net, obs, mask, iterations, EXPLORE), v_old, z_old)
        for layout, inplace in ((BATCH, False), (RING, True)):
            H.check(H.run(env, obs, mask, v_old, z_old, iterations, layout=layout, inplace=inplace, lead=1), exp, v_old if inplace else 0x5A5A,
                    (iterations, layout is RING))


# ---- argument errors ------------------------------------------------------------------------------------------------------------------
def call_with(lib, prefix, net, **over):
    """One call that must fail before it reads a row: made-up addresses, 64 bytes aligned and far apart."""
    a = dict(ev=net.struct(), iterations=16, explore=16, considered=16, gumbel_noise=1, visit_offset=50, scale=23, seed=0, env_base=0, call=0,
             obs=1 << 20, obs_pitch=117, mask=2 << 20, mask_pitch=54, visits_in=3 << 20, visits_out=3 << 20, visits_pitch=54, z_in=4 << 20,
             z_pitch=1, root_value_out=5 << 20, root_priors_out=6 << 20, action_out=7 << 20, nodes_out=8 << 20, drift_out=9 << 20,
             census_out=10 << 20, gumbel_out=11 << 20, n=4)
    a.update(over)
    ev = a.pop("ev")
    rc = getattr(lib, prefix + "reanalyse_gumbel")(None if ev is None else C.addressof(ev), *[a[k] for k in list(a)], None)
    return rc, getattr(lib, prefix + "last_error")().decode()


ERRORS_IN_ORDER = [  # each case breaks its own rule and every later one's: the earlier rule is reported
    (dict(ev=None), "NULL"),
    (dict(iterations=0), "iterations must be in [1, 512]"),
    (dict(explore=1025), "explore must be in [0, 1024]"),
    (dict(call=1 << 24), "call must be below 2^24"),
    (dict(n=-1), "n < 0"),
    (dict(env_base=(1 << 42) - 3), "env_base + n must not exceed 2^42"),
    (dict(considered=0), "considered must be in [1, 54]"),
    (dict(considered=55), "considered must be in [1, 54]"),
    (dict(gumbel_noise=2), "gumbel_noise must be 0 or 1"),
    (dict(visit_offset=256), "visit_offset must be in [0, 255]"),
    (dict(scale=65), "scale must be in [0, 64]"),
    (dict(obs_pitch=116), "obs_pitch must be at least 117"),
    (dict(mask_pitch=53), "mask_pitch must be at least 54"),
    (dict(visits_pitch=53), "visits_pitch must be at least 54"),
    (dict(z_pitch=0), "z_pitch must be at least 1"),
    (dict(obs=None), "obs must not be NULL"),
    (dict(visits_out=None, root_value_out=None, root_priors_out=None, action_out=None, nodes_out=None, drift_out=None, census_out=None,
          gumbel_out=None), "at least one output must be given"),
    (dict(gumbel_out=(1 << 20) + 116), "an output overlaps an input (only visits_in == visits_out may alias)"),
]


@pytest.mark.parametrize("flavour", ["host", "device"])
def test_argument_errors_in_their_stated_order(flavour):
    lib, prefix = (nat.cpu_raw(), "gbl_cpu_") if flavour == "host" else (nat.lib(), "gbl_")
    net = H.net64()
    broken = {}
    for k in range(len(ERRORS_IN_ORDER) - 1, -1, -1):              # from the last rule up: case k with every later case's breakage too
        over, why = ERRORS_IN_ORDER[k]
        broken = {**broken, **over}
        rc, msg = call_with(lib, prefix, net, **broken)
        assert rc == nat.ERR_ARG and why in msg, (flavour, k, why, msg)
        rc, msg = call_with(lib, prefix, net, **over)                # ... and on its own
        assert rc == nat.ERR_ARG and why in msg, (flavour, k, why, msg)
    assert call_with(lib, prefix, net, n=0, obs=None)[0] == 0         # n == 0 returns before the pointers
    assert call_with(lib, prefix, net, n=0, obs_pitch=1)[0] == nat.ERR_ARG
    assert call_with(lib, prefix, net, n=0, env_base=1 << 42)[0] == 0 and call_with(lib, prefix, net, n=0, env_base=(1 << 42) + 1)[0] == nat.ERR_ARG
    rc, msg = call_with(lib, prefix, net, gumbel_out=3 << 20)        # gumbel_out on visits_in's rows
    assert rc == nat.ERR_ARG and "overlaps" in msg
    if flavour == "device":                                          # the alignments, after every argument rule
        for over, why in ((dict(visits_in=(3 << 20) + 1, visits_out=(3 << 20) + 1), "visits_in must be 2-byte aligned"),
                          (dict(visits_in=None, visits_out=(3 << 20) + 1), "visits_out must be 2-byte aligned"),
                          (dict(root_value_out=(5 << 20) + 2), "4-byte aligned"), (dict(drift_out=(9 << 20) + 1), "4-byte aligned"),
                          (dict(gumbel_out=(11 << 20) + 1), "gumbel_out must be 2-byte aligned")):
            rc, msg = call_with(lib, prefix, net, **over)
            assert rc == nat.ERR_ALIGN and why in msg, (over, msg)
        rc, msg = call_with(lib, prefix, net, gumbel_out=(11 << 20) + 1, considered=0)
        assert rc == nat.ERR_ARG and "considered" in msg


# ---- the Python surface on the host flavour ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring():
    return GH.gumbel_ring(H.net64(), "cpu", prioritized=True)


def test_evaluator_reanalyse_on_a_batch_dict(world, ring):
    env = world[0][64]
    buf, ev = ring
    batch = buf.batch(48, symmetries=None, call=3, seed=1)
    before = {k: v.clone() for k, v in batch.items()}
    spec = dict(considered=8, noise=True, visit_offset=40, scale=20)
    out = ev.reanalyse(batch, iterations=16, explore=EXPLORE, census=True, gumbel=spec, seed=9, call=4, env_base=100)
    assert all(torch.equal(batch[k], before[k]) for k in before) and out["visits"] is not batch["visits"]
    assert set(out) == set(batch) | {"root_value", "drift", "census", "gumbel"}
    s = GRR.searched(env.net, before["observation"].numpy(), before["action_mask"].numpy(), 16, EXPLORE, 8, 1, 40, 20, 9, 100, 4)
    exp = GRR.reanalyse(s, before["visits"].numpy(), before["z"].numpy())
    GH.check({k: out[k].numpy() for k in ("visits", "root_value", "drift", "census", "gumbel")}, exp, before["visits"].numpy())
    assert out["gumbel"].dtype == torch.int16 and out["gumbel"].shape == (48, 54) and out["gumbel"].any()
    defaults = ev.reanalyse(batch, iterations=16, explore=EXPLORE, gumbel={})
    same = ev.reanalyse(batch, iterations=16, explore=EXPLORE, gumbel=dict(considered=16, noise=True, visit_offset=50, scale=23), seed=0, call=0, env_base=0)
    assert all(torch.equal(defaults[k], same[k]) for k in same) and "census" not in defaults
    # gumbel=None is the call it was
    old = ev.reanalyse(batch, iterations=16, explore=EXPLORE, census=True)
    s = RR.searched(env.net, before["observation"].numpy(), before["action_mask"].numpy(), 16, EXPLORE)
    H.check({k: old[k].numpy() for k in ("visits", "root_value", "drift", "census")}, RR.reanalyse(s, before["visits"].numpy(), before["z"].numpy()),
            before["visits"].numpy())
    assert "gumbel" not in old and set(old) == set(batch) | {"root_value", "drift", "census"}
    visits = batch["visits"]
    inplace = ev.reanalyse(batch, iterations=16, explore=EXPLORE, gumbel=spec, seed=9, call=4, env_base=100, out=visits)
    assert inplace["visits"] is visits and torch.equal(visits, out["visits"])
    for bad, why in ((dict(considered=0), "considered must be an integer in"), (dict(considered=55), "considered"), (dict(scale=65), "scale"),
                     (dict(visit_offset=-1), "visit_offset"), (dict(noise=2), "noise is True or False"), (dict(budget=3), "gumbel is a dict"),
                     (dict(considered=1.5), "considered")):
        with pytest.raises(ValueError, match=why):
            ev.reanalyse(batch, iterations=16, gumbel=bad)
    with pytest.raises(ValueError, match="gumbel is a dict"):
        ev.reanalyse(batch, iterations=16, gumbel=16)
    with pytest.raises(ValueError, match="call must be"):
        ev.reanalyse(batch, iterations=16, gumbel={}, call=1 << 24)
    with pytest.raises(ValueError, match="env_base"):
        ev.reanalyse(batch, iterations=16, gumbel={}, env_base=(1 << 42) - 3)
    with pytest.raises(ValueError, match="iterations"):
        ev.reanalyse(batch, iterations=513, gumbel={})


def test_ring_reanalyse_sets_priorities_from_the_new_drift(ring):
    buf, ev = ring
    state = buf.state_dict()
    live = buf.size
    spec = dict(considered=4, noise=True)
    plain = buf.reanalyse(ev, iterations=8, explore=EXPLORE, gumbel=spec, seed=2, call=1)
    assert (buf.priority[:live] == 1).all()
    rows = buf._visits[:live, :nat.ACTIONS].clone()
    buf.load_state_dict(state)
    out = buf.reanalyse(ev, iterations=8, explore=EXPLORE, census=True, prioritize=dict(floor=3, scale=5), gumbel=spec, seed=2, call=1)
    assert torch.equal(out["drift"], plain["drift"]) and (out["drift"] > 0).any() and torch.equal(buf._visits[:live, :nat.ACTIONS], rows)
    assert torch.equal(buf.priority[:live], (3 + 5 * out["drift"].clamp(min=0)).to(torch.int32)) and not buf.priority[live:].any()
    assert (buf.batch(64, call=1, prioritized=True)["index"][:, 0] >= 0).all()
    # g = the slot: the ring's call is the batch call on the live rows with env_base 0
    buf.load_state_dict(state)
    rowsd = {"observation": buf.observation[:live].contiguous(), "action_mask": buf.action_mask[:live].contiguous(),
             "visits": buf.visits[:live].contiguous(), "z": buf.z[:live].contiguous()}
    by_rows = ev.reanalyse(rowsd, iterations=8, explore=EXPLORE, gumbel=spec, seed=2, call=1, env_base=0)
    assert torch.equal(by_rows["visits"], rows) and torch.equal(by_rows["drift"], plain["drift"])
    buf.load_state_dict(state)
    for bad in (dict(considered=0), dict(what=1)):
        with pytest.raises(ValueError, match="gumbel"):
            buf.reanalyse(ev, iterations=8, gumbel=bad)
    empty = G.ReplayBuffer(16, "cpu").reanalyse(ev, census=True, gumbel={})
    assert empty["drift"].shape == empty["census"].shape == (0,)


def test_fit_with_gumbel_reanalysis(ring):
    buf, ev = ring
    spec = dict(evaluator=ev, iterations=8, explore=EXPLORE, gumbel=dict(considered=8), seed=11)
    a, b, c = (G.GobbletTrainer(hidden=64, device="cpu", seed=1) for _ in range(3))
    stats = buf.fit(a, 3, batch=64, symmetries=None, first_call=5, reanalyse=spec)
    hand, noises = [], []
    for i in range(3):
        rows = ev.reanalyse(buf.batch(64, symmetries=None, call=5 + i), 8, EXPLORE, gumbel=dict(considered=8), seed=11, call=5 + i)
        noises.append(rows["gumbel"].clone())
        hand.append(b.step(rows))
    assert torch.equal(stats, torch.stack(hand)) and torch.equal(a.params, b.params) and torch.isfinite(stats).all()
    # equal rows at two steps (the same draw of the ring) get fresh noise ...
    same_rows = buf.batch(64, symmetries=None, call=5)
    two = [ev.reanalyse(same_rows, 8, EXPLORE, gumbel=dict(considered=8), seed=11, call=5 + i) for i in range(2)]
    assert not torch.equal(two[0]["gumbel"], two[1]["gumbel"]) and torch.equal(two[0]["gumbel"], noises[0])
    # ... and without noise equal targets
    quiet = [ev.reanalyse(same_rows, 8, EXPLORE, gumbel=dict(considered=8, noise=False), seed=11, call=5 + i) for i in range(2)]
    assert torch.equal(quiet[0]["visits"], quiet[1]["visits"]) and not quiet[0]["gumbel"].any()
    # it composes with the prioritised loop
    state = buf.state_dict()
    stats = buf.fit(c, 2, batch=64, first_call=9, reanalyse=spec, prioritized=True, beta=(0.4, 1.0), priority=dict(scale=64.0, floor=1, cap=1 << 20))
    assert stats.shape == (2, 4) and torch.isfinite(stats).all()
    buf.load_state_dict(state)
    with pytest.raises(ValueError, match="reanalyse=dict"):
        buf.fit(a, 1, reanalyse=dict(evaluator=ev, noise=True))
    with pytest.raises(ValueError, match="seed goes with gumbel"):
        buf.fit(a, 1, reanalyse=dict(evaluator=ev, seed=3))
    with pytest.raises(ValueError, match="considered"):
        buf.fit(a, 1, reanalyse=dict(evaluator=ev, gumbel=dict(considered=99)))


def test_the_gumbel_reanalysis_example_runs_on_the_host_flavour():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("example_reanalyse_gumbel", os.path.join(root, "examples", "example_reanalyse_gumbel.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    out = ex.refresh("cpu", boards=32, plies=8, steps=2, batch=64, iterations=16, capacity=512)
    assert out["rows"] > 0 and out["evaluations"] > 0 and 0.0 < out["rows_per_evaluation"] <= 1.0
    assert sum(out["drift_histogram"]) == out["rows"] and 0.0 <= out["mean_drift"] <= 1.0
