"""gbl_symmetry_apply and gbl_training_batch on the MI355X (-m gpu): the kernels against the host flavour bit for bit (which
tests/test_symmetry.py holds to the restatement of the header and to the oracle), guard bytes around every output, subsets of the rows,
the device's own legal mask and observation commuting with the group, the argument errors, and one end-to-end case through the Python
surface.  Shapes: a lone board, a ragged tile on each side of 64, several tiles with a ragged tail, both trajectory layouts.
(`call` travels by value only -- it has no device-resident form -- so there is no captured-graph case here.)"""
import json
import os

import numpy as np
import pytest
import torch

from tests import symmetry_restatement as R
from tests.search_harness import G, replay_arg_errors  # noqa: F401  (G: the fixture)
from tests.test_symmetry import random_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD, JUNK = 64, 0x5A


class Guarded:
    """A device output of `shape` / `dtype` with GUARD junk bytes on both sides (the payload starts 16-byte aligned)."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), dtype
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        self.raw = torch.full((self.nbytes + 2 * GUARD,), JUNK, dtype=torch.uint8, device=DEV)

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def read(self):
        raw = self.raw.cpu().numpy()
        assert (raw[:GUARD] == JUNK).all() and (raw[GUARD + self.nbytes:] == JUNK).all(), "a guard byte was written"
        return raw[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_apply(lib, sym, agent, **rows):
    """gbl_symmetry_apply on the device: dict of numpy outputs, every one read back through its guards."""
    n = len(next(iter(rows.values())))
    ins = {k: dev(np.ascontiguousarray(v, R.DTYPES[k])) for k, v in rows.items()}
    outs = {k: Guarded(v.shape, R.DTYPES[k]) for k, v in rows.items()}
    codes = None if np.isscalar(sym) else dev(np.ascontiguousarray(sym, np.int16))
    ag = None if agent is None else dev(np.ascontiguousarray(agent, np.int8))
    pairs = []
    for k in R.ROWS:
        pairs += [ins[k].data_ptr() if k in ins else None, outs[k].ptr if k in outs else None]
    rc = lib.gbl_symmetry_apply(None if codes is None else codes.data_ptr(), int(sym) if codes is None else 0,
                                None if ag is None else ag.data_ptr(), *pairs, n, None)
    assert rc == 0, lib.gbl_last_error()
    torch.cuda.synchronize()
    return {k: o.read() for k, o in outs.items()}


def device_batch(lib, w, wd, batch, sym_mask, seed, sample_base, call, only=R.BATCH_OUT):
    """gbl_training_batch on the device window `wd` (the tensors of w): dict over `only`, read back through guards."""
    shapes = {"obs": ((batch, 117), np.int8), "mask": ((batch, 54), np.int8), "visits": ((batch, 54), np.int16), "z": ((batch,), np.int8),
              "index": ((batch, 2), np.int32), "sym": ((batch,), np.int16)}
    out = {k: Guarded(*shapes[k]) for k in only}
    rc = lib.gbl_training_batch(*[wd[k].data_ptr() for k in ("obs", "mask", "visits", "z", "done", "mover")], w["n"], w["plies"],
                                w["ply_stride"], w["tile_stride"], batch, sym_mask, seed, sample_base, call,
                                *[out[k].ptr if k in out else None for k in R.BATCH_OUT], None)
    assert rc == 0, lib.gbl_last_error()
    torch.cuda.synchronize()
    return {k: o.read() for k, o in out.items()}


def on_device(w):
    return {k: dev(v) for k, v in w.items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("n", [1, 63, 65, 4099])
def test_symmetry_apply_equals_host_flavour(G, n):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    rows = random_rows(n, seed=n)
    rng = np.random.default_rng(n + 1)
    agent = rng.integers(0, 2, n).astype(np.int8) * rng.choice(np.array([1, -1, 2, 127], np.int8), n)
    sym = rng.integers(0, 512, n)
    sym[:min(n, 512)] = rng.permutation(512)[:min(n, 512)]                      # (4 099 boards: every code)
    sym = (sym | rng.choice([0, -512], n)).astype(np.int16)                     # (only the low 9 bits are read)
    exp = R.run_apply(cpu, sym, agent, **rows)
    got = device_apply(lib, sym, agent, **rows)
    for k in R.ROWS:
        assert np.array_equal(got[k], exp[k]), k
    for subset in (("state",), ("obs",), ("visits", "actions"), ("mask", "priors"), ("actions",)):
        sub = {k: rows[k] for k in subset}
        ag = None if subset == ("state",) else agent
        got, exp = device_apply(lib, sym, ag, **sub), R.run_apply(cpu, sym, ag, **sub)
        assert set(got) == set(subset) and all(np.array_equal(got[k], exp[k]) for k in subset), subset
    for s in (0, 0b110101101):
        got, exp = device_apply(lib, s, agent, **rows), R.run_apply(cpu, s, agent, **rows)
        assert all(np.array_equal(got[k], exp[k]) for k in R.ROWS), s


def test_device_legal_mask_and_observation_commute(G):
    """gbl_legal_mask / gbl_observe of the image == the image of gbl_legal_mask / gbl_observe, on 4 099 masked-random boards."""
    n = 4099
    env = G.BatchedGobblet(n, DEV, auto_reset=True, seed=21)
    env.rollout(9)
    state, to_move = env.squares.clone(), env.to_move.clone()
    sym = torch.from_numpy(np.random.default_rng(5).integers(0, 512, n)).to(DEV)
    sym[:512] = torch.arange(512, device=DEV)
    lib = G._native.lib()
    mask, obs = torch.empty((n, 54), dtype=torch.int8, device=DEV), torch.empty((n, 117), dtype=torch.int8, device=DEV)
    g_mask, g_obs = torch.empty_like(mask), torch.empty_like(obs)
    G._native.check(lib.gbl_legal_mask(state.data_ptr(), to_move.data_ptr(), mask.data_ptr(), n, None))
    G._native.check(lib.gbl_observe(state.data_ptr(), to_move.data_ptr(), -1, obs.data_ptr(), n, None))
    img = G.symmetry.apply(sym, to_move, state=state, observation=obs, action_mask=mask)
    G._native.check(lib.gbl_legal_mask(img["state"].data_ptr(), to_move.data_ptr(), g_mask.data_ptr(), n, None))
    G._native.check(lib.gbl_observe(img["state"].data_ptr(), to_move.data_ptr(), -1, g_obs.data_ptr(), n, None))
    assert torch.equal(g_mask, img["action_mask"]) and torch.equal(g_obs, img["observation"])
    assert not torch.equal(g_mask, mask) and int(to_move.sum()) not in (0, n)


@pytest.mark.parametrize("boards,plies,layout", R.WINDOWS)
def test_training_batch_equals_host_flavour(G, boards, plies, layout):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    w = R.host_window(boards, plies, layout)
    wd = on_device(w)
    seed, base = 0x1234567890ABCDEF, (1 << 40) + 5
    for batch, sym_mask, call in ((1, 511, 0), (63, 7, 1), (65, 511, (1 << 26) - 1), (1000, 511, 2), (1000, 0, 2)):
        got, exp = device_batch(lib, w, wd, batch, sym_mask, seed, base, call), R.run_batch(cpu, w, batch, sym_mask, seed, base, call)
        R.same_batch(got, exp)
    got = device_batch(lib, w, wd, 200, 511, seed, base, 2, only=("visits", "index"))   # the other outputs NULL
    exp = R.run_batch(cpu, w, 200, 511, seed, base, 2)
    assert np.array_equal(got["visits"], exp["visits"]) and np.array_equal(got["index"], exp["index"])


def test_training_batch_edge_windows(G):
    lib, cpu = G._native.lib(), G._native.cpu_raw()
    none = R.synthetic_window(70, 5, np.zeros((5, 70), bool))
    valid = np.zeros((6, 65), bool)
    valid[1:, 64] = True
    ragged = R.synthetic_window(65, 6, valid)
    valid = np.zeros((2, 130), bool)
    valid[1, ::2] = True
    two = R.synthetic_window(130, 2, valid)
    for w, batch, sym_mask in ((none, 65, 511), (ragged, 300, 7), (two, 200, 511)):
        got = device_batch(lib, w, on_device(w), batch, sym_mask, 3, 0, 0)
        R.same_batch(got, R.run_batch(cpu, w, batch, sym_mask, 3, 0, 0))
    assert (got["index"][:, 0] != 0).all()


def test_argument_errors_replay_the_recorded_table(G, golden_dir):
    replay_arg_errors(json.load(open(os.path.join(golden_dir, "batch_arg_errors.json"))), flavours=("device",))
    torch.cuda.synchronize()


def test_collect_to_training_batch_end_to_end(G):
    """env.collect with the tree search on the device -> outcome_targets -> training_batch(1000), against the restatement run on the
    window copied back."""
    boards, plies = 200, 12
    env = G.BatchedGobblet(boards, DEV, auto_reset=True, seed=17, track_turn=True)
    traj = env.collect(plies, policies=("tree", "tree"), search=R.SEARCH)
    env.outcome_targets(traj)
    out = env.training_batch(traj, 1000, symmetries="all", call=6)
    assert all(v.device.type == "cuda" for v in out.values())
    w = R.window_of(traj, boards)
    exp, failed = R.training_batch(w, 1000, 511, 17, 0, 6)
    assert failed < 10
    for k, r in (("observation", "obs"), ("action_mask", "mask"), ("visits", "visits"), ("z", "z"), ("index", "index"), ("sym", "sym")):
        assert np.array_equal(out[k].cpu().numpy(), exp[r]), k
    z, visits = traj["z"][1:], traj["visits"][1:].float()
    keep = (z != G._native.Z_OPEN) & (traj["done"][:-1] == 0) & (visits.sum(-1) > 0)   # the trainer's keep set
    t, b = out["index"].long().T
    assert bool(keep[t - 1, b].all())
