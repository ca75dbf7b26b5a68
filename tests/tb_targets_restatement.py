"""The rule of include/gobblet_hip.h, "Tablebase targets", restated in numpy on top of a probe's (outcome, value, action) -- what
gbl_decode_obs + gbl_tb_probe give for the rows -- separately from the library's code.  A plain module."""
import numpy as np

Z_OPEN = NONE = -128
RESULT, SHORTEST = 0, 1


def sign(x):
    return (x > 0) - (x < 0)


def targets(outcome, value, action, mode, count, visits_in=None, z_in=None):
    """Per row: "written" (False: a skipped row, whose visits_out / z_out bytes stay as they were), "visits" int16 (n, 54), "z",
    "value", "outcome" (n, 54) and "census" int8."""
    n = len(value)
    out = {"written": np.ones(n, bool), "visits": np.zeros((n, 54), np.int16), "z": np.full(n, Z_OPEN, np.int8), "value": np.zeros(n, np.int8),
           "outcome": np.full((n, 54), NONE, np.int8), "census": np.full(n, -1, np.int8)}
    for r in range(n):
        if z_in is not None and int(z_in[r]) == Z_OPEN:
            out["written"][r] = False
            continue
        out["outcome"][r] = outcome[r]
        if int(action[r]) == -1:
            continue                                   # unlabelled: zero visits, z = Z_OPEN, census -1, value 0
        v = int(value[r])
        keeps = [a for a in range(54) if int(outcome[r, a]) != NONE and sign(int(outcome[r, a])) == sign(v)]
        short = [a for a in range(54) if int(outcome[r, a]) != NONE and int(outcome[r, a]) == v]
        for a in (keeps if mode == RESULT else short):
            out["visits"][r, a] = count
        out["z"][r], out["value"][r] = sign(v), v
        census = 0
        old = None if visits_in is None else [int(x) for x in visits_in[r]]
        if old is None or max(old) <= 0:
            census |= 4
        elif old.index(max(old)) in keeps:             # (list.index: the lowest index on ties)
            census |= 1
        if z_in is not None and int(z_in[r]) == sign(v):
            census |= 2
        out["census"][r] = census
    return out
