"""gbl_cpu_tb_targets (include/gobblet_hip.h, "Tablebase targets") against the restatement of its rule applied to gbl_cpu_decode_obs +
gbl_cpu_tb_probe, byte for byte through guard bytes: on the complete table of (2, 2, 0) and on a table of pseudo-random bytes over
(1, 1, 2) that holds every byte value.  Rows: sampled positions seen by player_1, their negatives seen by player_2, masked-random
full-inventory play (mostly no state of either inventory: unlabelled) and all-zero rows."""
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from gobblet_rl_amd import symmetry as S
from tests import tablebase_harness as H
from tests import tablebase_restatement as R
from tests import tb_targets_harness as TH
from tests import tb_targets_restatement as T

DEEP, WIDE, make_rows, old_targets = TH.DEEP, TH.WIDE, TH.make_rows, TH.old_targets


@pytest.fixture(scope="module")
def deep():
    host = H.Host(DEEP)
    table, counts = host.build()
    env = TH.HostEnv(DEEP, table)
    return env, make_rows(env.host, 31)


@pytest.fixture(scope="module")
def wide():
    env = TH.HostEnv(WIDE, TH.random_table(H.layout(WIDE)[0], 32))
    return env, make_rows(env.host, 33)


@pytest.fixture(params=["deep", "wide"])
def world(request, deep, wide):
    return deep if request.param == "deep" else wide


def masks_of(st, tm, seed):
    legal = TH.legal_mask(st, tm)
    rng = np.random.default_rng(seed)
    return {"null": None, "legal": legal, "subset": (rng.random(legal.shape) < 0.5).astype(np.int8) * 3, "empty": np.zeros_like(legal)}


def case(env, obs, mask, v_old, z_old, mode, count, what, **kw):
    exp = TH.expected(env, obs, mask, v_old, z_old, mode, count)
    inplace = kw.get("inplace", True)
    got = TH.run(env, obs, mask, v_old, z_old, mode, count, **kw)
    TH.check(got, exp, v_old if (inplace and v_old is not None) else 0x5A5A, z_old if (inplace and z_old is not None) else TH.JUNK, what)
    return got, exp


@pytest.mark.parametrize("mode", [T.RESULT, T.SHORTEST])
@pytest.mark.parametrize("count", [1, 600])
def test_every_source_and_mask_equals_the_restatement(world, mode, count):
    env, (obs, st, tm) = world
    v_old, z_old = old_targets(len(obs), 34)
    seen = set()
    for name, mask in masks_of(st, tm, 35).items():
        got, exp = case(env, obs, mask, v_old, z_old, mode, count, name)
        seen |= set(exp["census"].tolist())
        labelled = exp["census"] >= 0
        if name == "empty":
            assert not labelled.any()
        else:
            assert labelled[:240].sum() > 100 and (~labelled[240:-6]).sum() > 80 and not labelled[-6:].all()
            assert (got["visits"][labelled].sum(1) >= count).all() and got["visits"][exp["written"]].max() == count
    assert {-1, 0, 1, 2, 3, 4, 6} <= seen
    assert (z_old == nat.Z_OPEN).sum() > 20


def test_the_random_table_shows_ties_and_the_widest_results(wide):
    env, (obs, st, tm) = wide
    exp = TH.expected(env, obs, None, None, None, T.SHORTEST, 1)
    out = exp["outcome"][exp["census"] >= 0]
    assert {-127, 127} <= set(out.reshape(-1).tolist())
    assert ((exp["visits"] > 0).sum(1) > 1).any()                     # a tie inside S
    res = TH.expected(env, obs, None, None, None, T.RESULT, 1)
    assert ((res["visits"] > 0).sum(1) > (exp["visits"] > 0).sum(1)).any()  # R is wider than S somewhere


def test_a_result_beyond_the_byte_belongs_to_neither_set(wide):
    """A table byte of +-127 (no sweep writes one) gives c(a) = -+128: GBL_SOLVE_NONE as the probe's byte.  Such a candidate is in
    neither R nor S even where the row's value has its sign."""
    env, (obs, st, tm) = wide
    table = np.random.default_rng(48).choice(np.array([-127, -5, 127, 3], np.int8), len(env.table))
    odd = TH.HostEnv(WIDE, table)
    legal = TH.legal_mask(st, tm)
    for mode in (T.RESULT, T.SHORTEST):
        got, exp = case(odd, obs, legal, None, None, mode, 2, mode)
        beyond = (exp["outcome"] == T.NONE) & (legal != 0) & (exp["census"] >= 0)[:, None]
        assert (beyond.any(1) & (exp["value"] > 0)).sum() > 50 and not got["visits"][beyond].any()


def test_skipped_rows_keep_their_bytes_in_place_and_not(world):
    env, (obs, st, tm) = world
    v_old, z_old = old_targets(len(obs), 36)
    for inplace in (True, False):
        for layout in (TH.BATCH, TH.RING):
            case(env, obs, None, v_old, z_old, T.RESULT, 7, (inplace, layout is TH.RING), inplace=inplace, layout=layout)


def test_in_place_equals_separate_outputs(world):
    env, (obs, st, tm) = world
    v_old, z_old = old_targets(len(obs), 37)
    z_old[z_old == nat.Z_OPEN] = 0                                     # (no skipped row: every output byte is defined)
    mask = masks_of(st, tm, 38)["subset"]
    a = TH.run(env, obs, mask, v_old, z_old, T.SHORTEST, 5, inplace=True)
    b = TH.run(env, obs, mask, v_old, z_old, T.SHORTEST, 5, inplace=False)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_every_optional_pointer_null_in_turn(world):
    env, (obs, st, tm) = world
    v_old, z_old = old_targets(len(obs), 39)
    legal = TH.legal_mask(st, tm)
    for keep in (("value",), ("outcome",), ("census",), ()):
        case(env, obs, legal, v_old, z_old, T.RESULT, 2, keep, keep=keep)
    got, exp = case(env, obs, legal, None, z_old, T.RESULT, 2, "no visits_in")
    assert ((exp["census"] >= 0) <= ((exp["census"] & 4) != 0)).all()
    got, exp = case(env, obs, legal, v_old, None, T.RESULT, 2, "no z_in")
    assert exp["written"].all() and not (exp["census"][exp["census"] >= 0] & 2).any()
    case(env, obs, None, None, None, T.SHORTEST, 2, "no optional input")
    # visits_out NULL: z and the dense outputs as before, no visits row written
    exp = TH.expected(env, obs, legal, v_old, z_old, T.RESULT, 2)
    got = TH.run(env, obs, legal, v_old, z_old, T.RESULT, 2, inplace=False, give_visits_out=False)
    assert np.array_equal(got["z"], np.where(exp["written"], exp["z"], TH.JUNK)) and np.array_equal(got["census"], exp["census"])


@pytest.mark.parametrize("lead", [0, 1, 3])
def test_ring_pitches_odd_addresses_and_padding(world, lead):
    env, (obs, st, tm) = world
    v_old, z_old = old_targets(len(obs), 40)
    mask = masks_of(st, tm, 41)["legal"]
    for layout in (TH.BATCH, TH.RING):
        for inplace in (True, False):
            case(env, obs, mask, v_old, z_old, T.RESULT, 600, (lead, inplace), layout=layout, inplace=inplace, lead=lead)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_row_counts(world, n):
    env, (obs, st, tm) = world
    v_old, z_old = old_targets(len(obs), 42)
    pick = np.r_[0:n // 2, 240:240 + n - n // 2]
    for layout in (TH.BATCH, TH.RING):
        case(env, obs[pick], None, v_old[pick], z_old[pick], T.SHORTEST, 3, n, layout=layout)


def test_census_bits_on_hand_made_old_visits(deep):
    env, (obs, st, tm) = deep
    base = TH.expected(env, obs, None, None, None, T.RESULT, 1)
    keeps = base["visits"] > 0
    rows = np.nonzero((base["census"] >= 0) & (keeps.sum(1) < (base["outcome"] != T.NONE).sum(1)) & (keeps.sum(1) > 0))[0][:40]
    assert len(rows) == 40                                               # rows with candidates inside AND outside R
    obs4 = np.repeat(obs[rows], 5, axis=0)
    v = np.zeros((200, 54), np.int16)
    z = np.zeros(200, np.int8)
    for i, r in enumerate(rows):
        inside, outside = np.nonzero(keeps[r])[0], np.nonzero((base["outcome"][r] != T.NONE) & ~keeps[r])[0]
        v[5 * i, inside[0]], v[5 * i, outside[0]] = 9, 8                 # argmax inside R
        v[5 * i + 1, inside[0]], v[5 * i + 1, outside[0]] = 8, 9         # argmax outside R
        v[5 * i + 3, inside[-1]] = v[5 * i + 3, outside[0]] = 5          # a tie: the lowest index decides
        v[5 * i + 4, :] = -1                                             # nothing positive
        v[5 * i + 4, 0] = 0
        z[5 * i:5 * i + 5] = [base["z"][r], -base["z"][r] if base["z"][r] else 1, 0, base["z"][r], base["z"][r]]
    got, exp = case(env, obs4, None, v, z, T.RESULT, 1, "census")
    c = got["census"].reshape(40, 5)
    assert (c[:, 0] == 3).all() and (c[:, 1] == 0).all() and (c[:, 2] & 4).all() and (c[:, 4] == 6).all()
    tie_inside = np.array([np.nonzero(keeps[r])[0][-1] < np.nonzero((base["outcome"][r] != T.NONE) & ~keeps[r])[0][0] for r in rows])
    assert np.array_equal(c[:, 3] & 1, tie_inside.astype(np.int8)) and 0 < tie_inside.sum() < 40


# ---- symmetry -----------------------------------------------------------------------------------------------------------------
def image(s, agent, rows):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in rows.items()}
    out = S.apply(s, agent=torch.from_numpy(np.ascontiguousarray(agent, np.int8)), **t)
    return {k: v.numpy() for k, v in out.items()}


def sym_rows(env):
    """Quiet sampled positions of (2, 2, 0), both movers, with their legal masks and old visits that have one argmax."""
    st, tm = H.sample_boards(env.host, 300, 43, renumber=False)
    obs, mask = TH.observe(st, tm), TH.legal_mask(st, tm)
    rng = np.random.default_rng(44)
    v_old = np.stack([rng.permutation(54) for _ in range(len(st))]).astype(np.int16) * mask
    return st, tm, obs, mask, v_old, rng.choice(np.array([-1, 0, 1], np.int8), len(st))


def targets_commute(env, s, st, tm, obs, mask, v_old, z_old, rows, mode):
    got = TH.run(env, obs, mask, v_old, z_old, mode, 4)
    img = image(s, tm, {"observation": obs, "action_mask": mask, "visits": v_old})
    got_img = TH.run(env, img["observation"], img["action_mask"], img["visits"], z_old, mode, 4)
    moved = image(s, tm, {"visits": got["visits"]})["visits"]
    for k, a, b in (("visits", got_img["visits"], moved), ("z", got_img["z"], got["z"]), ("value", got_img["value"], got["value"]),
                    ("census", got_img["census"], got["census"])):
        assert np.array_equal(a[rows], b[rows]), (s, k, int((a[rows] != b[rows]).reshape(len(a[rows]), -1).any(1).sum()))


@pytest.mark.parametrize("mode", [T.RESULT, T.SHORTEST])
def test_targets_commute_with_the_piece_swaps(deep, mode):
    env, _ = deep
    st, tm, obs, mask, v_old, z_old = sym_rows(env)
    every = np.ones(len(st), bool)
    for s in range(0, 512, 8):                                           # bits 3-8: the 64 piece swaps, exact on every row
        targets_commute(env, s, st, tm, obs, mask, v_old, z_old, every, mode)


def both_colours_hold_a_line(cells):
    tops = [next((cells[9 * level + pos] for level in (2, 1, 0) if cells[9 * level + pos]), 0) for pos in range(9)]
    return len({tops[a] for a, b, c in R.LINES if tops[a] and tops[a] == tops[b] == tops[c]}) == 2


def a_successor_holds_lines_of_both_colours(U, cells):
    """... among the positions the two-ply table's answer looks at: after a move of the mover, and after the reply to a quiet one."""
    for q in R.moves(U, cells):
        if both_colours_hold_a_line(q) or (not R.winner(q) and any(both_colours_hold_a_line(g) for g in R.moves(U, R.swap(q)))):
            return True
    return False


def inventory_play_rows(n, plies, seed):
    """Boards of masked-random play with the pieces of (2, 2, 0) only, after each of `plies` ply counts: (state, to_move)."""
    rng = np.random.default_rng(seed)
    env = G.BatchedGobblet(n, "cpu", auto_reset=False, seed=seed)
    st, tm = [], []
    for ply in range(max(plies) + 1):
        live = ~env.done.numpy().astype(bool)
        if ply in plies:
            st.append(env.squares.numpy()[live].copy()), tm.append(env.to_move.numpy()[live].copy())
        m = env.action_mask.numpy().astype(float)
        m[:, 36:] = 0
        m[m.sum(1) == 0, 0] = 1                                           # (a frozen board consumes no action)
        env.step(torch.from_numpy(np.array([rng.choice(54, p=r / r.sum()) for r in m], np.int32)))
    return np.concatenate(st), np.concatenate(tm)


def test_targets_commute_with_the_squares_symmetries():
    """check_for_winner's last-line-decides rule is not symmetric where a move leaves lines of both colours; those rows are left out,
    and they must be at most 2 % of the set.  The table here is (2, 2, 0) after sweeps 0 and 1, whose answers look two plies ahead,
    so "no successor" covers exactly what an answer reads: the position after a move and after the reply.  The COMPLETE table is
    no ground for this test: such positions anywhere below a row reach its values, and the probe itself (gbl_cpu_tb_probe, as
    pinned) answers 67 of 295 sampled rows that pass the one-ply criterion differently from their images.  Rows: play with the
    inventory's pieces after 2 .. 8 plies, both movers."""
    host = H.Host(DEEP)
    table, counts = host.build(max_sweeps=1)
    env = TH.HostEnv(DEEP, table)
    st, tm = inventory_play_rows(60, (2, 3, 5, 6, 8), 46)
    obs, mask = TH.observe(st, tm), TH.legal_mask(st, tm)
    rng = np.random.default_rng(47)
    v_old = np.stack([rng.permutation(54) for _ in range(len(st))]).astype(np.int16) * mask
    z_old = rng.choice(np.array([-1, 0, 1], np.int8), len(st))
    U = R.Universe(DEEP)
    keep = np.array([not a_successor_holds_lines_of_both_colours(U, R.cells_of(st[b], int(tm[b]))) for b in range(len(st))])
    assert len(st) > 250 and 0 < (~keep).sum() <= 0.02 * len(st), ((~keep).sum(), len(st))
    values = TH.run(env, obs, mask, v_old, z_old, T.RESULT, 1)["value"]
    assert {-2, 0, 1} <= set(values.tolist()) and set(tm.tolist()) == {0, 1}
    for s in range(1, 8):
        for mode in (T.RESULT, T.SHORTEST):
            targets_commute(env, s, st, tm, obs, mask, v_old, z_old, keep, mode)


# ---- the Python surface and the recorded argument errors ------------------------------------------------------------------------
def test_tablebase_targets_on_a_batch_dict(deep):
    env, (obs, st, tm) = deep
    tb = G.Tablebase(DEEP, "cpu")
    tb.table.copy_(torch.from_numpy(env.table.copy()))
    v_old, z_old = old_targets(len(obs), 45)
    mask = TH.legal_mask(st, tm)
    batch = {"observation": torch.from_numpy(obs.copy()), "action_mask": torch.from_numpy(mask.copy()), "visits": torch.from_numpy(v_old.copy()),
             "z": torch.from_numpy(z_old.copy()), "index": torch.zeros((len(obs), 2), dtype=torch.int32)}
    with pytest.raises(ValueError, match="not complete"):
        tb.targets(batch)
    tb.complete = True
    visits, z = batch["visits"], batch["z"]
    out = tb.targets(batch, mode="shortest", count=9, census=True)
    assert out is batch and out["visits"] is visits and out["z"] is z
    exp = TH.expected(env, obs, mask, v_old, z_old, T.SHORTEST, 9)
    TH.check({"visits": visits.numpy(), "z": z.numpy(), "value": out["tb_value"].numpy(), "census": out["census"].numpy()}, exp, v_old, z_old)
    assert "census" not in tb.targets({k: v for k, v in batch.items() if k != "census"})
    for bad, why in (({k: v for k, v in batch.items() if k != "observation"}, "observation"), (dict(batch, z=batch["z"].to(torch.int16)), "z must be")):
        with pytest.raises(ValueError, match=why):
            tb.targets(bad)
    with pytest.raises(ValueError, match="mode"):
        tb.targets(batch, mode="best")
    with pytest.raises(ValueError, match="count"):
        tb.targets(batch, count=601)
    tb.complete = False
    tb.targets(batch, allow_incomplete=True)


def test_argument_errors_replay_the_recorded_table(golden_dir):
    table = json.load(open(os.path.join(golden_dir, "tb_targets_arg_errors.json")))
    assert len(table) > 30 and {c["fn"] for c in table} == {"tb_targets"}
    TH.replay_arg_errors(table)
