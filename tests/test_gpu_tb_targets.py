"""k_tb_targets on the MI355X (-m gpu) against the host flavour byte for byte (which tests/test_tb_targets.py holds to the restatement
of the header's rule), every array read back through guard bytes and padding: the (2, 2, 0) table built on the device and a table of
pseudo-random bytes over (1, 1, 2); one row, the rows around a wavefront's 64 and more rows than one pass of the capped grid; a
batch's pitches and the ring's; both modes; in place and not; odd addresses; skipped and unlabelled rows; a relabel right behind an
append on one stream; and the full inventory on 1 423^3 pseudo-random bytes against gbl_decode_obs + gbl_tb_probe on the device plus
the restatement, where successor indices lie above 2^31."""
import numpy as np
import pytest
import torch

from gobblet_rl_amd import _native as nat
from tests import symmetry_restatement as S
from tests import tablebase_harness as H
from tests import tb_targets_harness as TH
from tests import tb_targets_restatement as T
from tests.search_harness import G  # noqa: F401  (the fixture)
from tests.tb_targets_harness import DEEP, WIDE, make_rows, old_targets

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_ROWS = 4 * 4096   # rows one pass of the launch's grid takes (kTbTargetWaves x kTbTargetGroups)


class DevEnv:
    """The device flavour of one inventory with a table of the caller's (a device tensor): the mirror of tb_targets_harness.HostEnv."""
    prefix = "gbl_"

    def __init__(self, inventory, table):
        self.L, self.inv = nat.lib(), H.inv_array(inventory)
        self.aux, self.table = torch.zeros(nat.TB_AUX_BYTES, dtype=torch.uint8, device=DEV), table
        self.stream = nat.current_stream(DEV)
        assert self.L.gbl_tb_prepare(self.inv, self.aux.data_ptr(), self.stream) == 0
        self.aux_ptr, self.table_ptr = self.aux.data_ptr(), table.data_ptr()

    @staticmethod
    def upload(raw):
        return torch.from_numpy(raw).to(DEV)

    def error(self):
        return self.L.gbl_last_error()


@pytest.fixture(scope="module")
def worlds(G):
    """Per table: (device env, host env on the same bytes, rows)."""
    tb = G.Tablebase(DEEP, DEV)
    tb.build()
    assert tb.complete
    deep = (DevEnv(DEEP, tb.table), TH.HostEnv(DEEP, tb.table.cpu().numpy()))
    table = TH.random_table(H.layout(WIDE)[0], 32)
    wide = (DevEnv(WIDE, torch.from_numpy(table).to(DEV)), TH.HostEnv(WIDE, table))
    return {"deep": deep + (make_rows(deep[1].host, 31),), "wide": wide + (make_rows(wide[1].host, 33),)}


def same(dev, host, obs, mask, v_old, z_old, mode, count, what, **kw):
    got, exp = TH.run(dev, obs, mask, v_old, z_old, mode, count, **kw), TH.run(host, obs, mask, v_old, z_old, mode, count, **kw)
    assert set(got) == set(exp)
    for k in exp:
        assert got[k].tobytes() == exp[k].tobytes(), (what, k, np.argwhere(got[k] != exp[k])[:5])
    return exp


@pytest.mark.parametrize("name", ["deep", "wide"])
@pytest.mark.parametrize("mode", [T.RESULT, T.SHORTEST])
def test_kernel_equals_the_host_flavour(worlds, name, mode):
    dev, host, (obs, st, tm) = worlds[name]
    v_old, z_old = old_targets(len(obs), 50)
    legal = TH.legal_mask(st, tm)
    subset = (np.random.default_rng(51).random(legal.shape) < 0.5).astype(np.int8)
    for layout in (TH.BATCH, TH.RING):
        for inplace in (True, False):
            for lead in (0, 1):
                exp = same(dev, host, obs, subset, v_old, z_old, mode, 600, (layout is TH.RING, inplace, lead), layout=layout, inplace=inplace, lead=lead)
    census = exp["census"]
    skipped = z_old == nat.Z_OPEN
    assert skipped.sum() > 20 and ((census < 0) & ~skipped).sum() > 80 and (census >= 0).sum() > 80   # skipped, unlabelled and labelled rows
    for mask, v, z, keep in ((None, None, None, ("value", "outcome", "census")), (legal, v_old, None, ("census",)), (legal, None, z_old, ())):
        same(dev, host, obs, mask, v, z, mode, 1, "optional pointers", keep=keep)
    same(dev, host, obs, np.zeros_like(legal), v_old, z_old, mode, 1, "the empty mask")


@pytest.mark.parametrize("n", [1, 63, 64, 65, GRID_ROWS + 65])
def test_row_counts_around_a_wavefront_and_beyond_the_grid(worlds, n):
    dev, host, (obs, st, tm) = worlds["wide"]
    v_old, z_old = old_targets(len(obs), 52)
    pick = np.arange(n) * 7 % len(obs)
    for layout in ((TH.RING,) if n > GRID_ROWS else (TH.BATCH, TH.RING)):
        same(dev, host, obs[pick], None, v_old[pick], z_old[pick], T.RESULT, 3, n, layout=layout)


def test_a_relabel_behind_an_append_needs_no_synchronisation(G):
    """The ring wraps with the second append, so the live rows are all 150 slots whatever the counters say: append and relabel go out
    on one stream with nothing in between; the ring against the same steps on the host flavour."""
    rings = []
    for d in (DEV, "cpu"):
        tb = G.Tablebase(DEEP, d)
        tb.build()
        env = G.BatchedGobblet(130, d, auto_reset=True, seed=5, track_turn=True)
        traj = env.collect(6, policies=("tree", "tree"), search=S.SEARCH)
        env.outcome_targets(traj)
        buf = G.ReplayBuffer(150, d)
        buf.append(env, traj, tag=1)
        if d == DEV:
            torch.cuda.synchronize()
            with torch.cuda.stream(torch.cuda.Stream(DEV)):
                buf.append(env, traj, tag=2)
                census = tb._targets(150, buf._obs.data_ptr(), nat.REPLAY_OBS_PITCH, buf._meta.data_ptr(), nat.REPLAY_META_PITCH,
                                     buf._visits.data_ptr(), nat.REPLAY_VISITS_PITCH, buf._meta.data_ptr() + nat.REPLAY_META_Z,
                                     nat.REPLAY_META_PITCH, "result", 5, True, None, False)
                torch.cuda.current_stream().synchronize()
        else:
            buf.append(env, traj, tag=2)
            census = buf.relabel(tb, count=5, census=True)
        rings.append((buf, census))
    (gb, gc), (cb, cc) = rings
    assert gb.total == cb.total > 150 and torch.equal(gc.cpu(), cc) and (cc >= 0).sum() > 20 and (cc < 0).sum() > 20
    for a, b in ((gb._obs, cb._obs), (gb._visits, cb._visits), (gb._meta, cb._meta)):
        assert torch.equal(a.cpu(), b)
    assert torch.equal(gb.relabel(G.Tablebase(DEEP, DEV), allow_incomplete=True, census=True).cpu(), cb.relabel(G.Tablebase(DEEP, "cpu"), allow_incomplete=True, census=True))


def full_inventory_rows(G, n, plies):
    """Rows of masked-random full-inventory play after `plies` plies (host flavour), both movers, and for each the board one more
    random move leads to with its mover (a successor the probe looks up, unless that move ended the game)."""
    per = 3 * -(-n // len(plies))                                       # (about half the games are over by then)
    obs, child, child_tm, quiet = [], [], [], []
    for i, p in enumerate(plies):
        env = G.BatchedGobblet(per, "cpu", auto_reset=False, seed=60 + i)
        for _ in range(p):
            env.step(env.sample_actions())
        live = ~env.done.numpy().astype(bool)
        obs.append(env.observation.numpy().reshape(per, 117)[live].copy())
        env.step(env.sample_actions())
        child.append(env.squares.numpy()[live].copy()), child_tm.append(env.to_move.numpy()[live].copy()), quiet.append(~env.done.numpy().astype(bool)[live])
    order = np.random.default_rng(63).permutation(sum(len(x) for x in obs))[:n]
    return tuple(np.concatenate(x)[order] for x in (obs, child, child_tm, quiet))


def test_full_inventory_offsets_beyond_2_to_the_31(G):
    """4 096 rows on 1 423^3 pseudo-random bytes (no build: the rule reads whatever bytes there are) against the device composition
    gbl_decode_obs + gbl_tb_probe plus the restatement."""
    obs, child, child_tm, quiet = full_inventory_rows(G, 4096, tuple(range(6, 17)))
    n = len(obs)
    assert n == 4096 and set(child_tm.tolist()) == {0, 1}
    index = H.Host(H.FULL).index(child[quiet], child_tm[quiet])
    assert (index >= 0).all() and (index > 1 << 31).sum() > 10 and (index < 1 << 31).sum() > 10    # successors on both sides of 2^31
    gen = torch.Generator(device=DEV)
    gen.manual_seed(61)
    table = torch.randint(-128, 128, (H.FULL_POSITIONS,), dtype=torch.int8, device=DEV, generator=gen)
    dev = DevEnv(H.FULL, table)
    d_obs = torch.from_numpy(obs).to(DEV)
    state, who = torch.empty((n, 27), dtype=torch.int8, device=DEV), torch.empty(n, dtype=torch.int8, device=DEV)
    out = {"outcome": torch.empty((n, 54), dtype=torch.int8, device=DEV), "value": torch.empty(n, dtype=torch.int8, device=DEV),
           "action": torch.empty(n, dtype=torch.int32, device=DEV)}
    assert dev.L.gbl_decode_obs(d_obs.data_ptr(), state.data_ptr(), who.data_ptr(), n, dev.stream) == 0
    assert dev.L.gbl_tb_probe(dev.inv, dev.aux_ptr, dev.table_ptr, state.data_ptr(), who.data_ptr(), None, out["outcome"].data_ptr(),
                              out["value"].data_ptr(), out["action"].data_ptr(), n, dev.stream) == 0
    p = {k: v.cpu().numpy() for k, v in out.items()}
    assert (p["action"] >= 0).all() and len(set(p["value"].tolist())) > 20
    v_old, z_old = old_targets(n, 62)
    for mode, layout in ((T.RESULT, TH.BATCH), (T.SHORTEST, TH.RING)):
        exp = T.targets(p["outcome"], p["value"], p["action"], mode, 9, v_old, z_old)
        got = TH.run(dev, obs, None, v_old, z_old, mode, 9, layout=layout)
        TH.check(got, exp, v_old, z_old, mode)
