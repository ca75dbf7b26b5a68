"""The integer helpers of gbl_tree_search / gbl_collect_search (gobblet_device.h: tree_isqrt, tree_key, tree_order_key,
tree_final_key + tree_action_of, visits_pick, tree_pid) compiled for the host (tests/emu) against Python integers and numpy int64,
at the operand maxima the packed fields are sized for (1024 iterations of 256 playouts).  No GPU."""
import numpy as np

from tests import emu
from tests.test_selfplay_search import visits_draw
from tests.test_tree_policy import key, pid

KEY_BOUND = 1 << 20  # what tree_order_key relies on: (key + 1) << 6 | (63 - a) stays a 32-bit word and 0 stays "no child"


def test_isqrt_exhaustive():
    """Every x the helper is specified for ([0, 2^24)): r * r <= x < (r + 1) * (r + 1), in int64, no floating point."""
    chunk = 1 << 20
    for x0 in range(0, 1 << 24, chunk):
        x = np.arange(x0, x0 + chunk, dtype=np.int64)
        r = emu.tree_isqrt_range(x0, chunk).astype(np.int64)
        assert ((r * r <= x) & (x < (r + 1) * (r + 1))).all(), x0
    assert emu.tree_isqrt([0, 1, 3, 4, (1 << 24) - 1]).tolist() == [0, 1, 1, 2, 4095]


def check_keys(W, L, n, P, n_parent, X):
    got = emu.tree_key(W, L, n, P, n_parent, X)
    exp = [key(*t) for t in zip(W.tolist(), L.tolist(), n.tolist(), P.tolist(), n_parent.tolist(), X.tolist())]  # (Python integers)
    bad = np.flatnonzero(got.astype(np.int64) != np.array(exp, np.int64))
    assert not len(bad), [(W[i], L[i], n[i], P[i], n_parent[i], X[i], got[i], exp[i]) for i in bad[:5]]
    assert max(exp) < KEY_BOUND and int(got.max()) < KEY_BOUND
    return got


def test_key_corners():
    rows = []
    for n in (1, 2, 1023, 1024):
        for P in (1, 2, 3, 255, 256):
            nP = n * P
            for W, L in ((0, 0), (nP, 0), (0, nP), (nP // 2, nP - nP // 2)):
                for n_parent in (n, 1024):
                    for X in (0, 1, 16, 1023, 1024):
                        rows.append((W, L, n, P, n_parent, X))
    assert len(rows) == 4 * 5 * 4 * 2 * 5
    got = check_keys(*np.array(rows, np.int64).T)
    # the largest key there is: one visit, every game won, under a full parent at the largest explore
    assert int(got.max()) == key(256, 0, 1, 256, 1024, 1024) == 65536 + ((1024 * 3396) >> 3)


def test_key_random():
    rng = np.random.default_rng(20)
    m = 1 << 20  # (at least 10^6 tuples)
    n = rng.integers(1, 1025, m)
    P = rng.integers(1, 257, m)
    n_parent = rng.integers(n, 1025)
    W = rng.integers(0, n * P + 1)
    L = rng.integers(0, n * P - W + 1)
    X = rng.integers(0, 1025, m)
    assert m >= 10 ** 6 and (W + L <= n * P).all() and (n <= n_parent).all() and n_parent.max() == 1024
    check_keys(W, L, n, P, n_parent, X)


def lex_gt(a, b):
    """a > b for tuples of int64 arrays, lexicographically."""
    gt, eq = np.zeros(len(a[0]), bool), np.ones(len(a[0]), bool)
    for x, y in zip(a, b):
        gt |= eq & (x > y)
        eq &= x == y
    return gt, eq


def pairs(rng, m, values, lo, hi):
    """m pairs from [lo, hi]: half of them from a handful of `values` (ties and the extremes), half uniform."""
    out = []
    for _ in range(2):
        v = np.where(rng.random(m) < 0.5, rng.choice(np.array(values, np.int64), m), rng.integers(lo, hi + 1, m))
        out.append(v.astype(np.int64))
    return out


def test_order_key_orders_as_key_then_lower_action():
    rng = np.random.default_rng(21)
    m = 200000
    k1, k2 = pairs(rng, m, [0, 1, 65536, KEY_BOUND - 2, KEY_BOUND - 1], 0, KEY_BOUND - 1)
    a1, a2 = pairs(rng, m, [0, 1, 52, 53], 0, 53)
    o1, o2 = emu.tree_order_key(k1, a1).astype(np.int64), emu.tree_order_key(k2, a2).astype(np.int64)
    gt, eq = lex_gt((k1, -a1), (k2, -a2))
    assert gt.sum() > m // 4 and eq.sum() > 100 and ((k1 == k2) & (a1 != a2)).sum() > 1000  # (ties on the key are in)
    assert np.array_equal(o1 > o2, gt) and np.array_equal(o1 == o2, eq)
    assert (o1 > 0).all() and (o1 < (1 << 32)).all()  # 0 stays "no child"; nothing is lost from a 32-bit word
    assert np.array_equal(63 - (o1 & 63), a1)         # ... and the action comes back out of the low six bits


def test_final_key_orders_as_visits_then_margin_then_lower_action():
    rng = np.random.default_rng(22)
    m = 200000
    top = 1 << 18  # W, L <= 1024 * 256
    n1, n2 = pairs(rng, m, [1, 2, 1023, 1024], 1, 1024)
    w1, w2 = pairs(rng, m, [0, 1, top - 1, top], 0, top)
    l1, l2 = pairs(rng, m, [0, 1, top - 1, top], 0, top)
    a1, a2 = pairs(rng, m, [0, 1, 52, 53], 0, 53)
    twin = rng.random(m) < 0.1  # (children that differ in the action alone)
    n2, w2, l2 = np.where(twin, n1, n2), np.where(twin, w1, w2), np.where(twin, l1, l2)
    f1, f2 = emu.tree_final_key(n1, w1, l1, a1), emu.tree_final_key(n2, w2, l2, a2)
    gt, eq = lex_gt((n1, w1 - l1, -a1), (n2, w2 - l2, -a2))
    assert ((n1 == n2) & (w1 - l1 != w2 - l2)).sum() > 1000 and ((n1 == n2) & (w1 - l1 == w2 - l2) & (a1 != a2)).sum() > 100
    assert ((w1 - l1 == top) | (w1 - l1 == -top)).sum() > 100  # (both ends of the 2^18 bias)
    assert np.array_equal(f1 > f2, gt) and np.array_equal(f1 == f2, eq)
    assert (f1 > 0).all()
    assert np.array_equal(emu.tree_action_of(f1), a1) and np.array_equal(emu.tree_action_of(f2), a2)
    assert emu.tree_action_of([0]).tolist() == [-1]
    # the extremes themselves
    worst, best = emu.tree_final_key([1024, 1024], [0, top], [top, 0], [53, 0])
    assert int(worst) == (1024 << 32) | 10 and int(best) == (1024 << 32) | ((2 * top) << 6) | 63


def test_visits_pick_is_the_visit_proportional_draw():
    rng = np.random.default_rng(23)
    rows = [np.zeros(54, np.int32)]
    for a, v in ((0, 1), (0, 1024), (53, 1), (53, 1024), (17, 1)):  # one nonzero: at action 0, at action 53; sum 1
        r = np.zeros(54, np.int32)
        r[a] = v
        rows.append(r)
    for _ in range(40):  # sum 1024 (a finished search at the largest budget), spread over a few or over many actions
        r = np.zeros(54, np.int32)
        hit =rng.choice(54, int(rng.integers(2, 55)), replace=False)
        np.add.at(r, rng.choice(hit, 1024), 1)
        assert r.sum() == 1024
        rows.append(r)
    for _ in range(40):  # random rows, zeros among them
        rows.append((rng.integers(0, 200, 54) * (rng.random(54) < 0.5)).astype(np.int32))
    rs = [0, 1, 1 << 31, (1 << 32) - 1] + rng.integers(0, 1 << 32, 28).tolist()
    V = np.repeat(np.array(rows, np.int32), len(rs), axis=0)
    R = np.tile(np.array(rs, np.uint64), len(rows))
    got = emu.visits_pick(V, R)
    exp = np.array([visits_draw(v, int(r)) for v, r in zip(V, R)], np.int32)
    assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:5]
    assert (got[:len(rs)] == -1).all() and (exp[len(rs):2 * len(rs)] == 0).all() and (exp[3 * len(rs):5 * len(rs)] == 53).all()
    assert len(set(exp.tolist())) > 30


def test_pid_at_the_argument_limits():
    g, i, j = (1 << 42) - 1, 1023, 255
    got = emu.tree_pid([g, 0, 1, g], [i, 0, 0, 0], [j, 0, 255, 1])
    assert [int(x) for x in got] == [pid(g, i, j), 0, pid(1, 0, 255), pid(g, 0, 1)]
    assert pid(g, i, j) == (1 << 60) - 1  # (every id of the largest search fits 60 bits)
