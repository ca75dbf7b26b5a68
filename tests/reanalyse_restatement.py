"""The rule of gbl_reanalyse (include/gobblet_hip.h, "Reanalysis") restated in Python integers: the decode of the observation rows
(gbl_cpu_decode_obs, pinned by its own tests), tests/evaluator_restatement.py's restate_search left as it is, and the header's
sentences on the visits row, the drift and the census.  A plain module."""
import numpy as np

from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R

Z_OPEN = nat.Z_OPEN


def decode(obs):
    n = len(obs)
    obs = np.ascontiguousarray(obs, np.int8)
    st, tm = np.zeros((n, 27), np.int8), np.zeros(n, np.int8)
    if n:
        assert nat.cpu_raw().gbl_cpu_decode_obs(obs.ctypes.data, st.ctypes.data, tm.ctypes.data, n, None) == 0
    return st, tm


def argmax_key(row):
    """tb_visit_key's rule: the largest positive entry, the lowest index on ties; None where nothing is positive."""
    best = None
    for a, v in enumerate(row):
        v = int(v)
        if v > 0 and (best is None or v > best[0]):
            best = (v, a)
    return None if best is None else best[1]


def drift_of(old, new):
    """The total variation between the shares of `old` (entries <= 0 count 0) and `new`, in 1/1024; 1024 where nothing old is positive."""
    o = [max(int(x), 0) for x in old]
    n = [int(x) for x in new]
    so, sn = sum(o), sum(n)
    assert so <= 54 * 32767 and 0 < sn <= 512
    if so == 0:
        return 1024
    total = sum(abs(a * sn - b * so) for a, b in zip(o, n))
    assert total < 1 << 32 and 2 * so * sn < 1 << 32
    return (1024 * total) // (2 * so * sn)


def sign(x):
    return (x > 0) - (x < 0)


def searched(net, obs, mask, iterations, explore):
    """The part of the rule that does not look at the old targets, for every row as if none were skipped (the expensive part: the
    tests compute it once per (rows, mask, iterations) and share it)."""
    st, tm = decode(obs)
    visits, wins, losses, action, nodes, rootv, rootp = R.restate_search(net, st, tm, mask, iterations, explore)
    assert visits.max(initial=0) <= 32767
    return {"visits": visits.astype(np.int16), "action": action, "nodes": nodes, "root_value": rootv, "root_priors": rootp, "state": st, "to_move": tm}


def reanalyse(search, visits_old=None, z_old=None):
    """The outputs of gbl_reanalyse from `search` (searched(...) of the same rows) and the old targets: "written" (bool: the row is
    not skipped), "visits" (the new rows; whatever for a skipped row), and the six dense outputs."""
    n = len(search["action"])
    written = np.ones(n, bool) if z_old is None else np.asarray(z_old, np.int8) != Z_OPEN
    out = {"written": written, "visits": np.where(written[:, None], search["visits"], 0).astype(np.int16),
           "root_value": np.where(written, search["root_value"], 0).astype(np.int32),
           "root_priors": np.where(written[:, None], search["root_priors"], 0).astype(np.uint8),
           "action": np.where(written, search["action"], -1).astype(np.int32), "nodes": np.where(written, search["nodes"], 0).astype(np.int32),
           "drift": np.full(n, -1, np.int32), "census": np.full(n, -1, np.int8)}
    for r in range(n):
        if not written[r] or search["action"][r] < 0:          # skipped, or no candidate
            continue
        new = search["visits"][r]
        old = None if visits_old is None else visits_old[r]
        top_old = None if old is None else argmax_key(old)
        if old is not None:
            out["drift"][r] = drift_of(old, new)
        census = 0
        if top_old is not None and top_old == argmax_key(new):
            census |= 1
        if z_old is not None and int(z_old[r]) in (-1, 0, 1) and sign(int(search["root_value"][r])) == int(z_old[r]):
            census |= 2
        if top_old is None:
            census |= 4
        out["census"][r] = census
    return out
