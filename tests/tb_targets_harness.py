"""What tests/test_tb_targets.py and tests/test_gpu_tb_targets.py share: pitched, guarded buffers on the host (numpy) or the device
(torch), one call of gbl_tb_targets / gbl_cpu_tb_targets on them with every byte outside the rows checked, the row sources, and the
expectation: the restatement on top of the host flavour's gbl_cpu_decode_obs + gbl_cpu_tb_probe.  A plain module."""
import ctypes as C

import numpy as np

from gobblet_rl_amd import _native as nat
from tests import tablebase_harness as H
from tests import tb_targets_restatement as T

GUARD, JUNK = 64, 0x5A
BATCH = {"obs": 117, "mask": 54, "visits": 54, "z": 1}
RING = {"obs": nat.REPLAY_OBS_PITCH, "mask": nat.REPLAY_META_PITCH, "visits": nat.REPLAY_VISITS_PITCH, "z": nat.REPLAY_META_PITCH}


class Buf:
    """`dense` (n, row) laid out in rows `pitch` elements apart, `lead` bytes off a 64-byte boundary, junk in every other byte (the
    padding, and GUARD bytes on both sides).  upload: host bytes -> a device holder with data_ptr() (None: the host array itself)."""

    def __init__(self, dense, pitch, lead=0, upload=None, junk=JUNK):
        dense = np.ascontiguousarray(dense)
        self.n, self.row = dense.shape
        self.dtype, self.pitch, self.item = dense.dtype, pitch, dense.dtype.itemsize
        self.off = GUARD + lead
        raw = np.full(self.off + max(self.n, 1) * pitch * self.item + GUARD + 64, junk, np.uint8)
        base = raw.ctypes.data
        raw = raw[-base % 64:]                     # (the view starts on a 64-byte boundary: `lead` decides the alignment)
        self.payload = np.zeros(len(raw), bool)
        for r in range(self.n):
            at = self.off + r * pitch * self.item
            raw[at:at + self.row * self.item] = dense[r].view(np.uint8)
            self.payload[at:at + self.row * self.item] = True
        self.before, self.upload = raw.copy(), upload
        self.holder = raw if upload is None else upload(raw)

    @property
    def ptr(self):
        return (self.holder.ctypes.data if self.upload is None else self.holder.data_ptr()) + self.off

    def raw(self):
        return self.holder if self.upload is None else self.holder.cpu().numpy()

    def rows(self, also_written=None):
        """The rows as they are now; every byte outside them (less `also_written`, a bool mask over the raw bytes) must be unchanged."""
        raw = self.raw()
        frozen = ~self.payload if also_written is None else ~self.payload & ~also_written
        assert np.array_equal(raw[frozen], self.before[frozen]), "a byte outside the rows was written"
        return np.stack([raw[self.off + r * self.pitch * self.item:][:self.row * self.item].view(self.dtype) for r in range(self.n)]) \
            if self.n else np.zeros((0, self.row), self.dtype)


class HostEnv:
    """The host flavour of one inventory with a table of the caller's."""
    prefix, upload, stream = "gbl_cpu_", None, None

    def __init__(self, inventory, table):
        self.host = H.Host(inventory)
        self.L, self.inv, self.table = self.host.L, self.host.inv, np.ascontiguousarray(table, np.int8)
        self.aux_ptr, self.table_ptr = self.host.aux.ctypes.data, self.table.ctypes.data

    def error(self):
        return self.L.gbl_cpu_last_error()


def run(env, obs, mask=None, visits_old=None, z_old=None, mode=0, count=1, layout=BATCH, inplace=True, keep=("value", "outcome", "census"),
        lead=0, give_visits_out=True):
    """One call on fresh buffers.  visits_old / z_old: what the targets replace (None: visits_in / z_in are NULL and the output
    rows start as junk).  inplace: visits_out / z_out are the inputs' own pointers (where there are inputs).  The ring layout keeps z
    inside the mask's rows (byte 54 of 64), as ring_meta does.  Returns the rows read back: "visits", "z" and the kept dense outputs;
    every input row, every padding byte and every output not asked for is checked to be untouched."""
    n = len(obs)
    up, ring = env.upload, layout is RING
    lead2 = lead & ~1                                                  # (int16 rows: the device flavour wants them 2-byte aligned)
    b_obs = Buf(obs, layout["obs"], lead, up)
    junk_v, junk_z = np.full((n, 54), 0x5A5A, np.int16), np.full((n, 1), JUNK, np.int8)
    if ring:
        meta = np.full((n, 64), JUNK, np.int8)
        meta[:, :54] = 0 if mask is None else mask
        meta[:, 54] = JUNK if z_old is None else z_old
        b_meta = Buf(meta, 64, lead, up)
        mask_ptr, z_in_ptr = (None if mask is None else b_meta.ptr), (None if z_old is None else b_meta.ptr + 54)
        b_z = None
    else:
        b_mask = None if mask is None else Buf(mask, layout["mask"], 3 * lead, up)
        b_z = None if z_old is None else Buf(np.asarray(z_old, np.int8).reshape(n, 1), layout["z"], 5 * lead, up)
        mask_ptr, z_in_ptr = (None if b_mask is None else b_mask.ptr), (None if b_z is None else b_z.ptr)
    b_vin = None if visits_old is None else Buf(np.asarray(visits_old, np.int16), layout["visits"], lead2, up)
    b_vout = b_vin if (inplace and b_vin is not None) else Buf(junk_v, layout["visits"], lead2 + 2 * (lead != 0), up)
    if ring:
        b_zout, z_out_ptr = (b_meta, b_meta.ptr + 54) if (inplace or z_old is None) else (Buf(junk_z, layout["z"], 7 * lead, up), None)
    else:
        b_zout = b_z if (inplace and b_z is not None) else Buf(junk_z, layout["z"], 7 * lead, up)
        z_out_ptr = None
    z_out_ptr = b_zout.ptr if z_out_ptr is None else z_out_ptr
    dense = {"value": Buf(np.full((n, 1), JUNK, np.int8), 1, lead, up), "outcome": Buf(np.full((n, 54), JUNK, np.int8), 54, 3 * lead, up),
             "census": Buf(np.full((n, 1), JUNK, np.int8), 1, 5 * lead, up)}
    rc = getattr(env.L, env.prefix + "tb_targets")(
        env.inv, env.aux_ptr, env.table_ptr, b_obs.ptr, layout["obs"], mask_ptr, layout["mask"], None if b_vin is None else b_vin.ptr,
        b_vout.ptr if give_visits_out else None, layout["visits"], z_in_ptr, z_out_ptr, layout["z"], mode, count,
        *[dense[k].ptr if k in keep else None for k in ("value", "outcome", "census")], n, env.stream)
    assert rc == 0, env.error()
    got = {"visits": b_vout.rows()}
    assert np.array_equal(b_obs.rows(), obs), "the observation rows were written"
    if ring:
        now = b_meta.rows()
        assert np.array_equal(np.delete(now, 54, axis=1), np.delete(meta, 54, axis=1)), "mask, mover, tag or padding bytes of ring_meta were written"
        if b_zout is b_meta:
            got["z"] = now[:, 54].copy()
        else:
            assert np.array_equal(now[:, 54], meta[:, 54])
            got["z"] = b_zout.rows()[:, 0]
    else:
        got["z"] = b_zout.rows()[:, 0]
        if b_mask is not None:
            assert np.array_equal(b_mask.rows(), mask)
        if b_z is not None and b_zout is not b_z:
            assert np.array_equal(b_z.rows()[:, 0], z_old)
    if b_vin is not None and b_vout is not b_vin:
        assert np.array_equal(b_vin.rows(), visits_old)
    if not give_visits_out:
        assert np.array_equal(got["visits"], b_vout.before[b_vout.payload].view(np.int16).reshape(n, 54)), "visits_out was NULL and rows were written"
    for k, b in dense.items():
        rows = b.rows()
        if k in keep:
            got[k] = rows if k == "outcome" else rows[:, 0]
        else:
            assert (rows.view(np.uint8) == JUNK).all(), k
    return got


def expected(host_env, obs, mask=None, visits_old=None, z_old=None, mode=0, count=1):
    """The restatement applied to gbl_cpu_decode_obs + gbl_cpu_tb_probe (both pinned by their own tests), merged with what the output
    rows held before: a skipped row keeps its bytes (the inputs' when in place, junk otherwise -- see merge)."""
    n = len(obs)
    obs = np.ascontiguousarray(obs, np.int8)
    st, tm = np.zeros((n, 27), np.int8), np.zeros(n, np.int8)
    if n:
        assert host_env.L.gbl_cpu_decode_obs(obs.ctypes.data, st.ctypes.data, tm.ctypes.data, n, None) == 0
    p = host_env.host.probe(host_env.table, st, tm, mask) if n else {"outcome": np.zeros((0, 54), np.int8), "value": np.zeros(0, np.int8),
                                                                      "action": np.zeros(0, np.int32)}
    exp = T.targets(p["outcome"], p["value"], p["action"], mode, count, visits_old, z_old)
    exp["probe"], exp["state"], exp["to_move"] = p, st, tm
    return exp


def check(got, exp, visits_before, z_before, what=""):
    """got against exp; a skipped row must still hold visits_before / z_before (arrays, or scalars for junk fills)."""
    w = exp["written"]
    vb = np.broadcast_to(np.asarray(visits_before, np.int16), got["visits"].shape)
    zb = np.broadcast_to(np.asarray(z_before, np.int8), got["z"].shape)
    assert np.array_equal(got["visits"], np.where(w[:, None], exp["visits"], vb)), (what, "visits")
    assert np.array_equal(got["z"], np.where(w, exp["z"], zb)), (what, "z")
    for k in ("value", "outcome", "census"):
        if k in got:
            assert np.array_equal(got[k], exp[k]), (what, k, np.argwhere(got[k] != exp[k])[:5])


# ---- row sources ------------------------------------------------------------------------------------------------------------------
def observe(state, to_move):
    state, to_move = np.ascontiguousarray(state, np.int8), np.ascontiguousarray(to_move, np.int8)
    obs = np.zeros((len(state), 117), np.int8)
    assert nat.cpu_raw().gbl_cpu_observe(state.ctypes.data, to_move.ctypes.data, -1, obs.ctypes.data, len(state), None) == 0
    return obs


def position_rows(host, n, seed):
    """n sampled positions observed as player_1, then the same boards negated and observed as player_2: (obs (2n, 117), state, to_move)."""
    idx = np.random.default_rng(seed).integers(0, host.positions, n)
    st = host.position(idx)
    st = np.concatenate([st, -st]).astype(np.int8)
    tm = np.repeat(np.array([0, 1], np.int8), n)
    return observe(st, tm), st, tm


def random_play_rows(n, plies, seed):
    """Boards of masked-random full-inventory play after each of `plies` ply counts, both movers: (obs, state, to_move)."""
    import gobblet_rl_amd as G
    obs, st, tm = [], [], []
    per = -(-n // len(plies))
    for i, p in enumerate(plies):
        env = G.BatchedGobblet(per, "cpu", auto_reset=False, seed=seed + i)
        for _ in range(p):
            env.step(env.sample_actions())
        live = ~env.done.numpy().astype(bool)
        obs.append(env.observation.numpy().reshape(per, 117)[live].copy()), st.append(env.squares.numpy()[live].copy()), tm.append(env.to_move.numpy()[live].copy())
    obs, st, tm = np.concatenate(obs), np.concatenate(st), np.concatenate(tm)
    return obs[:n], st[:n], tm[:n]


DEEP, WIDE = (2, 2, 0), (1, 1, 2)


def make_rows(host, seed):
    """(obs, state, to_move) of the four sources, and where each starts."""
    p_obs, p_st, p_tm = position_rows(host, 120, seed)
    r_obs, r_st, r_tm = random_play_rows(160, (1, 2, 3, 4, 6, 9), seed + 1)
    z = np.zeros((6, 117), np.int8)
    obs = np.concatenate([p_obs, r_obs, z])
    st, tm = np.concatenate([p_st, r_st, np.zeros((6, 27), np.int8)]), np.concatenate([p_tm, r_tm, np.zeros(6, np.int8)])
    return obs, st, tm


def old_targets(n, seed):
    """Search-like old visits (some rows all zero, some negative entries) and old z (some GBL_Z_OPEN: skipped rows)."""
    rng = np.random.default_rng(seed)
    v = (rng.integers(0, 40, (n, 54)) * (rng.random((n, 54)) < 0.3)).astype(np.int16)
    v[rng.random(n) < 0.1] = 0
    v[rng.random(n) < 0.05] = -3
    z = rng.choice(np.array([-1, 0, 1, nat.Z_OPEN], np.int8), n, p=[0.3, 0.2, 0.3, 0.2])
    return v, z


def random_table(positions, seed):
    """Pseudo-random bytes holding every byte value: ties, +-126 / +-127 and GBL_TB_TERMINAL children occur."""
    t = np.random.default_rng(seed).integers(-128, 128, positions).astype(np.int8)
    assert len(set(t.tolist())) == 256
    return t


def legal_mask(state, to_move):
    state, to_move = np.ascontiguousarray(state, np.int8), np.ascontiguousarray(to_move, np.int8)
    m = np.zeros((len(state), 54), np.int8)
    assert nat.cpu_raw().gbl_cpu_legal_mask(state.ctypes.data, to_move.ctypes.data, m.ctypes.data, len(state), None) == 0
    return m


def replay_arg_errors(table, flavours=("device", "host")):
    """Every case of tests/golden/tb_targets_arg_errors.json (the format of tablebase_arg_errors.json; no pointer is ever read)."""
    libs = {"device": (nat.lib, "gbl_"), "host": (nat.cpu_raw, "gbl_cpu_")}
    for c in table:
        inv = None if c["inventory"] is None else H.inv_array(c["inventory"])
        args = [inv if x == "inv" else x for x in c["args"]]
        for flavour in flavours:
            if c[flavour] is None:
                continue
            lib, prefix = libs[flavour][0](), libs[flavour][1]
            rc, msg = c[flavour]
            assert getattr(lib, prefix + c["fn"])(*args) == rc, (flavour, c["case"])
            if rc:
                assert getattr(lib, prefix + "last_error")().decode() == msg, (flavour, c["case"])
