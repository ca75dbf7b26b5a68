"""A Python restatement of the gbl_evaluator / gbl_evaluate / gbl_tree_search_eval text of include/gobblet_hip.h on the oracle's
board functions (test infrastructure; written from the header, not from the device code), the seeded weight sets the evaluator
tests share, and the ctypes plumbing to run either flavour on host arrays."""
import ctypes as C
import math

import numpy as np

import oracle

from gobblet_rl_amd import _native as nat

P = 128
T = [int(math.floor(65536 * 2.0 ** (-k / 16) + 0.5)) for k in range(16)]
EVAL_NAMES = ("priors", "value", "logits")
SEARCH_NAMES = ("visits", "wins", "losses", "action", "nodes", "root_value", "root_priors")


class Net:
    """The four arrays in the header's layouts (w2 as [H / 4][56][4]) and the three shifts."""

    def __init__(self, w1, b1, w2, b2, shift1, shift_p, shift_v):
        self.hidden = int(w1.shape[1])
        assert w1.shape == (117, self.hidden) and b1.shape == (self.hidden,) and w2.shape == (self.hidden // 4, 56, 4) and b2.shape == (56,)
        self.w1, self.b1 = np.ascontiguousarray(w1, np.int8), np.ascontiguousarray(b1, np.int32)
        self.w2, self.b2 = np.ascontiguousarray(w2, np.int8), np.ascontiguousarray(b2, np.int32)
        self.shift1, self.shift_p, self.shift_v = int(shift1), int(shift_p), int(shift_v)
        # element (j, k) = weight of hidden unit j for output k
        self.w2_jk = self.w2.transpose(0, 2, 1).reshape(self.hidden, 56).astype(np.int64)

    def struct(self, arrays=None):
        """gbl_evaluator over host arrays (or over `arrays`: four objects with data_ptr(), e.g. device tensors)."""
        ptrs = [a.ctypes.data for a in (self.w1, self.b1, self.w2, self.b2)] if arrays is None else [a.data_ptr() for a in arrays]
        return nat.Evaluator(*ptrs, self.hidden, self.shift1, self.shift_p, self.shift_v)


def random_net(hidden, seed, shift1=1, shift_p=9, shift_v=9):
    """Ordinary random int8 weights.  6 to 21 rows of uniform int8 weights sum to a few hundred either way: after shift1 = 1 some
    hidden units are clamped at 0, some at 127 and some lie in between (the tests count them)."""
    rng = np.random.default_rng(seed)
    return Net(rng.integers(-128, 128, (117, hidden), dtype=np.int8), rng.integers(-300, 300, hidden).astype(np.int32),
               rng.integers(-128, 128, (hidden // 4, 56, 4), dtype=np.int8), rng.integers(-(1 << 16), 1 << 16, 56).astype(np.int32),
               shift1, shift_p, shift_v)


def extreme_net(hidden, sign1, sign2, shift1=0, shift_p=0, shift_v=0):
    """The extremes: every w1 +127 (sign1 > 0) or -128 with b1 at +-2^20 of that sign, every w2 +127 (sign2 > 0) or -128 with b2 at
    +-2^24 of that sign -- the largest sums the layers can reach."""
    return Net(np.full((117, hidden), 127 if sign1 > 0 else -128, np.int8), np.full(hidden, sign1 * (1 << 20), np.int32),
               np.full((hidden // 4, 56, 4), 127 if sign2 > 0 else -128, np.int8), np.full(56, sign2 * (1 << 24), np.int32),
               shift1, shift_p, shift_v)


def zero_net(hidden):
    return Net(np.zeros((117, hidden), np.int8), np.zeros(hidden, np.int32), np.zeros((hidden // 4, 56, 4), np.int8), np.zeros(56, np.int32),
               0, 0, 0)


def in_int32(x):
    assert -(1 << 31) <= int(np.min(x)) and int(np.max(x)) < (1 << 31)
    return x


def hidden_sums(net, s, side):
    """b1_j + the weight rows of the set observation bytes, before the shift (the tests count the clamped units from it)."""
    x = np.asarray(oracle.observe(s, side, side)["observation"], np.int64).reshape(117)
    assert set(np.unique(x).tolist()) <= {0, 1} and x.sum() <= 21
    return in_int32(net.b1.astype(np.int64) + net.w1[x == 1].astype(np.int64).sum(0))


def outputs(net, s, side):
    h = np.clip(hidden_sums(net, s, side) >> net.shift1, 0, 127)
    return in_int32(net.b2.astype(np.int64) + h @ net.w2_jk)


def value_of(net, o):
    return int(min(max(int(o[54]) >> net.shift_v, -128), 128))


def priors_of(net, o, cand):
    """cand: bool[54], not empty."""
    pi = np.zeros(54, np.uint8)
    acts = [int(a) for a in np.flatnonzero(cand)]
    l = {a: int(o[a]) >> net.shift_p for a in acts}
    top = max(l.values())
    e = {}
    for a in acts:
        d = min(top - l[a], 255)
        e[a] = T[d & 15] >> (d >> 4)
    total = sum(e.values())
    for a in acts:
        pi[a] = 1 + (e[a] * 254) // total
        assert 1 <= pi[a] <= 255
    return pi


def candidates(s, side, mask_row=None):
    cand = oracle.legal_mask(s, side) != 0
    if mask_row is not None:
        cand = cand & (np.asarray(mask_row) != 0)
    return cand


def restate_evaluate(net, state, to_move, mask=None):
    n = len(state)
    pri, val, log = np.zeros((n, 54), np.uint8), np.zeros(n, np.int32), np.zeros((n, 56), np.int32)
    for b in range(n):
        side = int(to_move[b] != 0)
        o = outputs(net, state[b], side)
        log[b], val[b] = o, value_of(net, o)
        cand = candidates(state[b], side, None if mask is None else mask[b])
        if cand.any():
            pri[b] = priors_of(net, o, cand)
    return pri, val, log


class Node:
    def __init__(self, parent, s, side, term, cand):
        self.parent, self.s, self.side, self.term, self.cand = parent, s, side, term, cand
        self.children = {}
        self.n = self.W = self.L = 0
        self.pi = None


def key(v, a, explore):
    c = v.children.get(a)
    if c is not None:
        mean, nc = ((c.W - c.L + c.n * P) << 15) // (c.n * P), c.n
    else:
        mean, nc = 32768, 0
    return mean + ((explore * int(v.pi[a]) * math.isqrt(v.n << 8)) >> 5) // (1 + nc)


def restate_search(net, state, to_move, mask, iterations, explore):
    """The contract, one iteration at a time.  (A node remembers its position: the header's nodes replay it from the root.)"""
    n = len(state)
    visits, wins, losses = (np.zeros((n, 54), np.int32) for _ in range(3))
    action, nodes, rootv = np.full(n, -1, np.int32), np.ones(n, np.int32), np.zeros(n, np.int32)
    rootp = np.zeros((n, 54), np.uint8)
    for b in range(n):
        mover = int(to_move[b] != 0)
        cand0 = candidates(state[b], mover, None if mask is None else mask[b])
        o = outputs(net, state[b], mover)
        rootv[b] = value_of(net, o)
        if not cand0.any():
            continue
        root = Node(None, state[b], mover, 0, [int(a) for a in np.flatnonzero(cand0)])
        root.pi = priors_of(net, o, cand0)
        rootp[b] = root.pi
        for _ in range(iterations):
            v = root
            while not v.term:  # 1. select
                a = max(v.cand, key=lambda x: (key(v, x, explore), -x))
                if a in v.children:
                    v = v.children[a]
                    continue
                s = oracle.play_turn(v.s, v.side, a)  # 2. expand
                w = oracle.check_for_winner(s)
                mine = w if v.side == 0 else -w
                side = 1 - v.side
                legal = oracle.legal_mask(s, side) != 0
                term = 1 if mine > 0 else 2 if mine < 0 else (0 if legal.any() else 3)
                c = Node(v, s, side, term, [int(x) for x in np.flatnonzero(legal)])
                v.children[a] = c
                nodes[b] += 1
                if term == 0:
                    oc = outputs(net, s, side)
                    c.pi = priors_of(net, oc, legal)
                    q = value_of(net, oc)
                    c.leaf = [max(-q, 0), max(q, 0)]
                v = c
                break
            if v.term:
                wl = [P if v.term == 1 else 0, P if v.term == 2 else 0]
            else:
                wl = list(v.leaf)
            while v.parent is not None:  # 3. back up
                v.n, v.W, v.L = v.n + 1, v.W + wl[0], v.L + wl[1]
                wl.reverse()
                v = v.parent
            root.n += 1
        for a, c in root.children.items():
            visits[b, a], wins[b, a], losses[b, a] = c.n, c.W, c.L
        action[b] = max(sorted(root.children), key=lambda a: (root.children[a].n, root.children[a].W - root.children[a].L, -a))
    return visits, wins, losses, action, nodes, rootv, rootp


# ---- either flavour on host arrays ---------------------------------------------------------------------------------------------------
def _in(state, to_move, mask):
    st, tm = np.ascontiguousarray(state, np.int8), np.ascontiguousarray(to_move, np.int8)
    mk = None if mask is None else np.ascontiguousarray(mask, np.int8)
    return st, tm, mk


def run_evaluate(lib, net, state, to_move, mask=None, logits=True):
    """gbl_cpu_evaluate through the host flavour's raw handle: (priors, value, logits)."""
    st, tm, mk = _in(state, to_move, mask)
    n = len(st)
    pri, val = np.full((n, 54), 99, np.uint8), np.full(n, -7, np.int32)
    log = np.full((n, 56), -7, np.int32) if logits else None
    ev = net.struct()
    rc = lib.gbl_cpu_evaluate(st.ctypes.data, tm.ctypes.data, None if mk is None else mk.ctypes.data, C.addressof(ev), pri.ctypes.data,
                              val.ctypes.data, None if log is None else log.ctypes.data, n, None)
    assert rc == 0, lib.gbl_cpu_last_error()
    return pri, val, log


def run_search(lib, net, state, to_move, mask, iterations, explore):
    """gbl_cpu_tree_search_eval through the host flavour's raw handle: the seven outputs."""
    st, tm, mk = _in(state, to_move, mask)
    n = len(st)
    out = [np.full((n, 54), -7, np.int32) for _ in range(3)] + [np.full(n, -7, np.int32) for _ in range(3)] + [np.full((n, 54), 99, np.uint8)]
    ev = net.struct()
    rc = lib.gbl_cpu_tree_search_eval(st.ctypes.data, tm.ctypes.data, None if mk is None else mk.ctypes.data, C.addressof(ev), iterations,
                                      explore, *[o.ctypes.data for o in out], n, None)
    assert rc == 0, lib.gbl_cpu_last_error()
    return tuple(out)


def same(got, exp, names):
    for name, g, e in zip(names, got, exp):
        assert g.dtype == e.dtype and np.array_equal(g, e), (name, np.argwhere(g != e)[:5])
