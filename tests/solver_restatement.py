"""The contract of gbl_solve (include/gobblet_hip.h) restated as a plain full-width recursion over the oracle's play_turn,
check_for_winner and legal_mask: no pruning, no code shared with the library (test infrastructure; slow on purpose).  Also the
position sets the CPU and the GPU tests of the solver share."""
import functools

import numpy as np

import oracle

NONE, MAX_DEPTH = -128, 6


def rank(c):
    return 64 - c if c > 0 else (0 if c == 0 else -64 - c)


def result(squares, s, a, r):
    """c(a): side s (0 / 1) plays the legal action a with r >= 1 plies left."""
    after = oracle.play_turn(squares, s, a)
    w = oracle.check_for_winner(after)
    me = -1 if s else 1
    if w == me:
        return 1
    if w == -me:
        return -1
    if r == 1:
        return 0
    u = value(after, 1 - s, r - 1)
    if u == 0:
        return 0
    return -(u + 1) if u > 0 else -u + 1


def value(squares, s, r):
    """V(position, s, r)."""
    best = None
    for a in np.flatnonzero(oracle.legal_mask(squares, s)):
        c = result(squares, s, int(a), r)
        if best is None or rank(c) > rank(best):
            best = c
    return 0 if best is None else best


def solve(state, to_move, mask, depth):
    """(outcome int8 (n, 54), value int8 (n,), action int32 (n,)) of the contract."""
    n = len(state)
    outcome, val, act = np.full((n, 54), NONE, np.int8), np.zeros(n, np.int8), np.full(n, -1, np.int32)
    for b in range(n):
        s = int(to_move[b] != 0)
        cand = oracle.legal_mask(state[b], s) != 0
        if mask is not None:
            cand &= np.asarray(mask[b]) != 0
        best = None
        for a in np.flatnonzero(cand):  # ascending: a later action replaces the best only with a larger rank
            c = result(state[b], s, int(a), depth)
            outcome[b, a] = c
            if best is None or rank(c) > rank(best):
                best, act[b] = c, a
        val[b] = 0 if best is None else best
    return outcome, val, act


def play(seq, first=0):
    """The board after a sequence of actions from the empty board, the sides alternating from `first`; (state, mover)."""
    s = np.zeros(27, np.int8)
    for i, a in enumerate(seq):
        who = (first + i) & 1
        assert oracle.legal_mask(s, who)[a], (seq, i)
        s = oracle.play_turn(s, who, a)
    return s, (first + len(seq)) & 1


@functools.lru_cache(maxsize=None)
def rollout_positions(per_ply, seed=11, plies=range(25)):
    """Masked-random positions (oracle.batch_rollout with auto-reset, so nobody holds a line): per_ply boards after t plies for every
    t of `plies`, board b of a ply on the generator of board b; the empty board first.  (state, to_move), read-only."""
    st, tm = [np.zeros((1, 27), np.int8)], [np.zeros(1, np.int8)]
    for t in plies:
        s, m, d = oracle.batch_reset(per_ply)
        if t:
            oracle.batch_rollout(s, m, d, seed + t, 0, 0, t, want_obs=False, want_mask=False)
        st.append(s)
        tm.append(m)
    st, tm = np.ascontiguousarray(np.concatenate(st)), np.ascontiguousarray(np.concatenate(tm))
    assert not oracle.batch_winner(st).any()
    st.setflags(write=False)
    tm.setflags(write=False)
    return st, tm


# ---- the position sets the tests of the solver share (tests/test_solver.py, tests/test_gpu_solver.py) ----------------------------
WIN_SEQ, WIN_ACTION = (0, 3, 10, 13), 20                  # player_1 holds squares 0 and 1; piece 3 to square 2 completes the row
UNCOVER_SEQ, UNCOVER_ACTION = (0, 5, 23, 12, 10, 22), 26  # player_1's piece 3 covers player_2's line 3-4-5; moving it uncovers it
# depth 3 in pure Python is ~1 s a position: two dozen of the sample (rollout_positions(2): board 2 t - 1 + j is board j after t plies)
D3 = (1, 5, 9, 12, 13, 16, 19, 21, 23, 26, 28, 31, 34, 36, 37, 40, 41, 43, 46, 47, 48, 49)
# late positions of the large sample whose trees stay small (forced lines): two forced losses in 4 and the one with the fewest moves
LATE = (1433, 1577, 2683)
# ... and three whose verdicts change late: unproven at depth 5 and lost in 6; won in 5; unproven throughout
DEEP = (2001, 2044, 2479)

# A win in TWO by zugzwang: a quiet move after which every move of the other side loses at once (each of their movable pieces is
# pinned on a covered line), so u = -1 and c = +2 -- the best a quiet move can give, which no random rollout of 700 000 boards held.
# Three boards around one such node, ZUG_NODE (player_2 to move): action 38 is the +2, and the LOWER action 35 a +3, so a search
# that stops at the first +3 gets the node wrong.
#   [0] ZUG_ROOT, player_1 to move: action 36 leads to ZUG_NODE -- the node sits at the REPLY level (c(36) = -3 at depth 4);
#   [1] ZUG_NODE itself, player_2 to move: +2 and +3 side by side among the root's results at depth 3;
#   [2] ZUG_DEEP, player_2 to move: action 22, then player_1's 49, lead to ZUG_NODE -- the node sits one ply deeper, inside the
#       serial recursion (c(22) = +4 at depth 5; stopping at the +3 gives +5).
ZUG_ROOT = (-2, -1, 0, 0, 1, 0, 2, 0, 0, 0, 0, 3, -4, -3, 0, 4, 0, 0, 0, -5, 0, 5, 6, 0, -6, 0, 0)
ZUG_DEEP = (-2, -1, 0, 0, 1, 0, 2, 0, 0, 0, 0, 3, -4, 0, 0, 4, 0, 0, 5, -5, 0, 0, 0, 0, -6, 0, 0)
ZUG_ROOT_ACTION, ZUG_DEEP_ACTIONS, ZUG_WIN_IN_2, ZUG_WIN_IN_3 = 36, (22, 49), 38, 35


@functools.lru_cache(maxsize=None)
def zugzwang():
    """(state (3, 27), to_move (3,)) of ZUG_ROOT, ZUG_NODE, ZUG_DEEP; both ways to ZUG_NODE are checked to arrive there."""
    root, deep = np.array(ZUG_ROOT, np.int8), np.array(ZUG_DEEP, np.int8)
    node = oracle.play_turn(root, 0, ZUG_ROOT_ACTION)
    via = oracle.play_turn(oracle.play_turn(deep, 1, ZUG_DEEP_ACTIONS[0]), 0, ZUG_DEEP_ACTIONS[1])
    assert np.array_equal(node, via) and oracle.legal_mask(deep, 1)[ZUG_DEEP_ACTIONS[0]]
    st, tm = np.ascontiguousarray([root, node, deep], np.int8), np.array([0, 1, 1], np.int8)
    assert not oracle.batch_winner(st).any()
    st.setflags(write=False)
    tm.setflags(write=False)
    return st, tm


def hand_built():
    """(state, to_move) of the boards built by hand: a win in 1 (WIN_ACTION completes a row) and a board with a move that loses at
    once (UNCOVER_ACTION lifts a piece off the opponent's line)."""
    (sw, mw), (su, mu) = play(WIN_SEQ), play(UNCOVER_SEQ)
    return np.array([sw, su], np.int8), np.array([mw, mu], np.int8)


@functools.lru_cache(maxsize=None)
def sample():
    """The positions of the restatement tests: the empty board, two masked-random boards after every ply 0 .. 24, the hand-built."""
    st, tm = rollout_positions(2)
    hs, hm = hand_built()
    st, tm = np.concatenate([st, hs]), np.concatenate([tm, hm])
    st.setflags(write=False)
    tm.setflags(write=False)
    return st, tm


@functools.lru_cache(maxsize=None)
def late(idx=LATE):
    st, tm = rollout_positions(120, seed=3)
    idx = np.array(idx)
    return np.ascontiguousarray(st[idx]), np.ascontiguousarray(tm[idx])
