"""The rule of gbl_reanalyse_gumbel (include/gobblet_hip.h, "Reanalysis with the Gumbel root rule") restated in Python integers, composed
from the two restatements it names: the decode and the row handling of tests/reanalyse_restatement.py, the Gumbel root search of
tests/gumbel_restatement.py (board id env_base + r, q = call), and the header's sentences on the target bytes in the visits' place and
the drift's 64-bit sum.  A plain module."""
import numpy as np

from tests import gumbel_restatement as GR
from tests import reanalyse_restatement as RR

Z_OPEN = RR.Z_OPEN
MAX_SN, MAX_SO = 54 * 255, 54 * 32767


def drift_of(old, new):
    """gbl_reanalyse's quotient over the target bytes, in exact integers: a single term fits 32 bits, the sum and the divisor need not."""
    o = [max(int(x), 0) for x in old]
    n = [int(x) for x in new]
    so, sn = sum(o), sum(n)
    assert so <= MAX_SO and 0 < sn <= MAX_SN
    if so == 0:
        return 1024
    terms = [abs(a * sn - b * so) for a, b in zip(o, n)]
    assert all(a * sn < 1 << 32 and b * so < 1 << 32 for a, b in zip(o, n))
    total = sum(terms)
    assert total <= 2 * so * sn and 1024 * total < 1 << 64
    return (1024 * total) // (2 * so * sn)


def searched(net, obs, mask, iterations, explore, considered, noise, visit_offset, scale, seed=0, env_base=0, call=0):
    """The part of the rule that does not look at the old targets, for every row as if none were skipped: row r is board env_base + r."""
    st, tm = RR.decode(obs)
    _, _, _, action, nodes, rootv, rootp, target, gum = GR.restate_search_gumbel(net, st, tm, mask, iterations, explore, considered, noise,
                                                                                 visit_offset, scale, seed, env_base, call)
    return {"visits": target.astype(np.int16), "action": action, "nodes": nodes, "root_value": rootv, "root_priors": rootp,
            "gumbel": gum.astype(np.int16), "state": st, "to_move": tm}


def reanalyse(search, visits_old=None, z_old=None):
    """The outputs of gbl_reanalyse_gumbel from `search` (searched(...) of the same rows) and the old targets: "written" (bool: the row is
    not skipped), "visits" (the new rows; whatever for a skipped row), and the seven dense outputs."""
    n = len(search["action"])
    written = np.ones(n, bool) if z_old is None else np.asarray(z_old, np.int8) != Z_OPEN
    out = {"written": written, "visits": np.where(written[:, None], search["visits"], 0).astype(np.int16),
           "root_value": np.where(written, search["root_value"], 0).astype(np.int32),
           "root_priors": np.where(written[:, None], search["root_priors"], 0).astype(np.uint8),
           "action": np.where(written, search["action"], -1).astype(np.int32), "nodes": np.where(written, search["nodes"], 0).astype(np.int32),
           "drift": np.full(n, -1, np.int32), "census": np.full(n, -1, np.int8),
           "gumbel": np.where(written[:, None], search["gumbel"], 0).astype(np.int16)}
    for r in range(n):
        new = search["visits"][r]
        if not written[r] or not new.any():                    # skipped, or no candidate (a candidate's byte is at least 1)
            assert not written[r] or search["action"][r] == -1
            continue
        old = None if visits_old is None else visits_old[r]
        top_old = None if old is None else RR.argmax_key(old)
        if old is not None:
            out["drift"][r] = drift_of(old, new)
        census = 0
        if top_old is not None and top_old == RR.argmax_key(new):  # (the largest target byte, the lowest index on ties: not the decision)
            census |= 1
        if z_old is not None and int(z_old[r]) in (-1, 0, 1) and RR.sign(int(search["root_value"][r])) == int(z_old[r]):
            census |= 2
        if top_old is None:
            census |= 4
        out["census"][r] = census
    return out
