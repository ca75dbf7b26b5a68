"""The exact tablebase restated from the text of include/gobblet_hip.h ("Exact tablebase") in plain Python and numpy.  Nothing here
calls the library.  Two independent routes to the same bytes:

  * ``V(U, cells, r)``: the recursive definition of gbl_solve's value on mover-relative positions, with a memo;
  * ``build(U)``: the sweeps over a whole universe at once (arrays over positions, one column of successors per move slot).

A position is a tuple of 27 cells (level-major, 9 * level + pos), each 0 empty / 1 own (the mover's) / 2 other."""
import functools

import numpy as np

TERMINAL = -128
MAX_SWEEP = 126
LINES = ((0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6))  # board.py:135-153, in the reference's order


def rank(c):
    """The shortest win, then the unproven, then the longest loss."""
    return 128 - c if c > 0 else (-128 - c if c < 0 else 0)


def parent(u):
    """c(a) from u = V of the position after a, for the other side."""
    return 0 if u == 0 else (-(u + 1) if u > 0 else 1 - u)


def digits(t):
    return tuple((t // 3 ** pos) % 3 for pos in range(9))


class Universe:
    """The positions of one inventory: the admissible level configurations in ascending ternary order, the index and its inverse."""

    def __init__(self, inventory):
        self.c = tuple(int(c) for c in inventory)
        assert len(self.c) == 3 and all(0 <= c <= 2 for c in self.c)
        self.levels = [[t for t in range(3 ** 9) if digits(t).count(1) <= c and digits(t).count(2) <= c] for c in self.c]
        self.code = [{t: i for i, t in enumerate(lv)} for lv in self.levels]
        self.L = [len(lv) for lv in self.levels]
        self.positions = self.L[0] * self.L[1] * self.L[2]

    def cells(self, index):
        assert 0 <= index < self.positions
        codes = (index % self.L[0], index // self.L[0] % self.L[1], index // (self.L[0] * self.L[1]))
        return tuple(d for level in range(3) for d in digits(self.levels[level][codes[level]]))

    def index(self, cells):
        """The index, or -1 where a level holds more cells of a colour than the inventory has pieces."""
        codes = []
        for level in range(3):
            t = sum(cells[9 * level + pos] * 3 ** pos for pos in range(9))
            if t not in self.code[level]:
                return -1
            codes.append(self.code[level][t])
        return (codes[2] * self.L[1] + codes[1]) * self.L[0] + codes[0]


def swap(cells):
    return tuple((0, 2, 1)[t] for t in cells)


def winner(cells):
    """check_for_winner() on the tops: 1 own, 2 other, 0 nobody; the LAST matching line decides (board.py:183-194)."""
    tops = [next((cells[9 * level + pos] for level in (2, 1, 0) if cells[9 * level + pos]), 0) for pos in range(9)]
    w = 0
    for line in LINES:
        if tops[line[0]] and tops[line[0]] == tops[line[1]] == tops[line[2]]:
            w = tops[line[0]]
    return w


def moves(U, cells):
    """The positions after each move of the mover (still as the mover sees them), in any order."""
    for level in range(3):
        free = [pos for pos in range(9) if not any(cells[9 * above + pos] for above in range(level, 3))]
        own = [pos for pos in range(9) if cells[9 * level + pos] == 1]
        sources = [pos for pos in own if not any(cells[9 * above + pos] for above in range(level + 1, 3))]
        if len(own) < U.c[level]:
            sources.append(None)  # the reserve
        for src in sources:
            for dst in free:
                q = list(cells)
                if src is not None:
                    q[9 * level + src] = 0
                q[9 * level + dst] = 1
                yield tuple(q)


def state_of(cells):
    """The contract state of a position with player_1 to move: own cells positive, the lowest piece number on the lowest cell."""
    row = np.zeros(27, np.int8)
    for level in range(3):
        n = {1: 0, 2: 0}
        for pos in range(9):
            t = cells[9 * level + pos]
            if t:
                row[9 * level + pos] = (2 * level + 1 + n[t]) * (1 if t == 1 else -1)
                n[t] += 1
    return row


def cells_of(state, to_move):
    """A concrete board as the side to move sees it."""
    own = 1 if not to_move else -1
    return tuple(0 if v == 0 else (1 if (v > 0) == (own > 0) else 2) for v in (int(x) for x in state))


def V_factory(U):
    """V(cells, r) of gbl_solve's text on the positions of U, memoised: r plies left, the mover to move."""
    @functools.lru_cache(maxsize=None)
    def V(cells, r):
        best = None
        for q in moves(U, cells):
            w = winner(q)
            if w == 1:
                c = 1
            elif w == 2:
                c = -1
            elif r == 1:
                c = 0
            else:
                c = parent(V(swap(q), r - 1))
            if best is None or rank(c) > rank(best):
                best = c
        return 0 if best is None else best
    return V


def outcomes(U, table, state, to_move, mask=None):
    """The probe's three outputs for one concrete board of the inventory, from a table (r = infinity): (int8[54], value, action)."""
    out = np.full(54, -128, np.int8)
    cells = cells_of(state, to_move)
    sign = -1 if to_move else 1
    best = None
    exist = all(v == 0 or 2 * (i // 9) + 1 <= abs(int(v)) <= 2 * (i // 9) + U.c[i // 9] for i, v in enumerate(state))
    if exist and U.index(cells) >= 0:  # (a state of the inventory: only pieces that exist, no more cells of a colour than pieces)
        for a in range(54):
            piece, pos = a // 9, a % 9
            level, which = piece // 2, piece % 2
            if which >= U.c[level] or (mask is not None and not mask[a]):
                continue
            number = sign * (piece + 1)
            where = [i for i in range(27) if state[i] == number]
            if any(state[9 * above + pos] for above in range(level, 3)):
                continue  # the cell holds a piece of this size or larger
            if where and any(state[9 * above + where[0] % 9] for above in range(where[0] // 9 + 1, 3)):
                continue  # the piece is covered
            q = list(cells)
            if where:
                q[where[0]] = 0
            q[9 * level + pos] = 1
            w = winner(tuple(q))
            if w:
                c = 1 if w == 1 else -1
            else:
                u = int(table[U.index(swap(tuple(q)))])
                c = parent(u) if u != TERMINAL else 0
            out[a] = c
            if best is None or rank(c) > rank(int(out[best])):
                best = a
    return out, (0 if best is None else int(out[best])), (-1 if best is None else best)


# ---- the sweeps over a whole universe --------------------------------------------------------------------------------------------------
def _winner_arrays(own, oth):
    """winner over arrays of per-level cell sets: +1 own, -1 other, 0."""
    occ = [own[level] | oth[level] for level in range(3)]
    top_own = own[2] | (own[1] & ~occ[2]) | (own[0] & ~occ[2] & ~occ[1])
    top_oth = oth[2] | (oth[1] & ~occ[2]) | (oth[0] & ~occ[2] & ~occ[1])
    w = np.zeros(own[0].shape, np.int8)
    for line in LINES:
        m = sum(1 << pos for pos in line)
        w = np.where((top_own & m) == m, 1, np.where((top_oth & m) == m, -1, w)).astype(np.int8)
    return w


def build(U, max_sweeps=None):
    """(table int8[positions] after the sweeps, [bytes written non-zero by sweep 0, 1, ...]); stops after the first sweep that decides
    nothing (that sweep's 0 is the last count) or after sweep `max_sweeps`."""
    N = U.positions
    assert N < 1 << 31
    idx = np.arange(N, dtype=np.int64)
    codes = [idx % U.L[0], idx // U.L[0] % U.L[1], idx // (U.L[0] * U.L[1])]
    stride = [1, U.L[0], U.L[0] * U.L[1]]
    tern_of = np.array([sum(3 ** pos for pos in range(9) if m >> pos & 1) for m in range(512)], np.int64)
    code_of = []
    for level in range(3):
        r = np.full(3 ** 9, -1, np.int64)
        r[U.levels[level]] = np.arange(U.L[level])
        code_of.append(r)
    own, oth = [], []
    for level in range(3):
        t = np.array(U.levels[level], np.int64)[codes[level]]
        o, x = np.zeros(N, np.int64), np.zeros(N, np.int64)
        for pos in range(9):
            d = t % 3
            t = t // 3
            o |= (d == 1).astype(np.int64) << pos
            x |= (d == 2).astype(np.int64) << pos
        own.append(o)
        oth.append(x)
    table = np.where(_winner_arrays(own, oth) != 0, TERMINAL, 0).astype(np.int8)
    counts = [int((table != 0).sum())]
    rows = np.nonzero(table == 0)[0]
    own, oth = [o[rows] for o in own], [x[rows] for x in oth]
    occ = [own[level] | oth[level] for level in range(3)]
    swapped = [code_of[level][tern_of[oth[level]] + 2 * tern_of[own[level]]] * stride[level] for level in range(3)]
    total = swapped[0] + swapped[1] + swapped[2]
    child, now = [], []  # per move slot: the successor's index (-1: none) and the immediate result (2: not a move)
    for level in range(3):
        if U.c[level] == 0:
            continue
        above = np.zeros(len(rows), np.int64)
        for j in range(level + 1, 3):
            above |= occ[j]
        dest = ~(above | occ[level]) & 511
        count = sum((own[level] >> pos) & 1 for pos in range(9))
        sources, rest = [(np.zeros(len(rows), np.int64), count < U.c[level])], own[level].copy()
        for _ in range(U.c[level]):
            bit = rest & -rest
            rest = rest & ~bit
            sources.append((bit, (bit != 0) & ((bit & above) == 0)))
        for bit, can in sources:
            for pos in range(9):
                legal = can & ((dest >> pos) & 1 != 0)
                new = (own[level] & ~bit) | (1 << pos)
                w = _winner_arrays([new if j == level else own[j] for j in range(3)], oth)
                succ = total - swapped[level] + code_of[level][tern_of[oth[level]] + 2 * tern_of[np.where(legal, new, 0)]] * stride[level]
                child.append(np.where(legal & (w == 0), succ, -1).astype(np.int32))
                now.append(np.where(legal, w, 2).astype(np.int8))
    child, now = np.stack(child), np.stack(now)
    k = 0
    while max_sweeps is None or k < max_sweeps:
        k += 1
        assert k <= MAX_SWEEP, "the build would need sweep 127"
        u = table[np.maximum(child, 0)].astype(np.int16)
        u = np.where((child >= 0) & (np.abs(u) >= 1) & (np.abs(u) <= k - 1), u, 0)
        c = np.where(now == 2, 0, np.where(now != 0, now, np.where(u > 0, -(u + 1), np.where(u < 0, 1 - u, 0)))).astype(np.int16)
        key = np.where(now == 2, 0, np.where(c > 0, 128 - c, np.where(c < 0, -128 - c, 0)) + 128)
        best = key.max(axis=0)
        r = best.astype(np.int16) - 128
        value = np.where(best == 0, 0, np.where(r > 0, 128 - r, np.where(r < 0, -128 - r, 0)))
        hit = np.abs(value) == k
        table[rows[hit]] = value[hit]
        counts.append(int(hit.sum()))
        if not hit.any():
            break
        keep = ~hit
        rows, child, now = rows[keep], child[:, keep], now[:, keep]
    return table, counts
