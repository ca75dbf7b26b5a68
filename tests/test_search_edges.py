"""gbl_tree_search / gbl_collect_search at the budgets their packed fields are sized for (1024 iterations of 256 playouts: W and L up
to 2^18 next to the action in one word, int16 visits, 18-bit values), host flavour against the Python restatements (no GPU).  The
restatement can afford these budgets on positions whose leaves are decided by the move into them: such leaves play no games."""
import os
import re

import numpy as np
import pytest

import oracle

from gobblet_rl_amd import _native as nat
from tests.search_harness import replay_arg_errors, run, same
from tests.test_playout_policy import UNCOVER_ACTION, UNCOVER_SEQ, WIN_ACTION, WIN_SEQ, play
from tests.test_selfplay_search import collect, restate_collect
from tests.test_selfplay_search import same as same_collect
from tests.test_tree_policy import restate

I_MAX, P_MAX, M_MAX = 1024, 256, 255
FULL = I_MAX * P_MAX  # 2^18: every game of every iteration
EXPLORES = (0, 16, 1024)
# the largest ids there are: env_base + n = 2^42, call = 2^24 - 1
SEED, ENV_BASE, CALL = 9, (1 << 42) - 3, (1 << 24) - 1


def saturated_boards():
    """Three boards and their root masks: (a) only the winning move, (b) only the move that uncovers the opponent's line, (c) the
    winning move and one other legal move that decides nothing."""
    (sw, mw), (su, mu) = play(WIN_SEQ), play(UNCOVER_SEQ)
    other = next(int(a) for a in np.flatnonzero(oracle.legal_mask(sw, mw))
                 if a != WIN_ACTION and oracle.check_for_winner(oracle.play_turn(sw, mw, int(a))) == 0)
    st, tm = np.array([sw, su, sw], np.int8), np.array([mw, mu, mw], np.int8)
    mask = np.zeros((3, 54), np.int8)
    mask[0, WIN_ACTION] = mask[1, UNCOVER_ACTION] = mask[2, WIN_ACTION] = mask[2, other] = 1
    assert oracle.legal_mask(su, mu)[UNCOVER_ACTION] and oracle.legal_mask(sw, mw)[WIN_ACTION]
    return st, tm, mask, other


_TREE = {}


def saturated_tree_expectation(explore, playouts=P_MAX):
    """restate() of the three boards at (1024, playouts, 255, explore), computed once per process (the GPU tests share it)."""
    if (explore, playouts) not in _TREE:
        st, tm, mask, _ = saturated_boards()
        exp = restate(st, tm, mask, I_MAX, playouts, M_MAX, explore, SEED, ENV_BASE, CALL)
        for a in exp:
            a.setflags(write=False)
        _TREE[(explore, playouts)] = exp
    return _TREE[(explore, playouts)]


def check_saturated_tree(got, explore, playouts=P_MAX):
    """The outputs of a (1024, playouts, 255, explore) search of saturated_boards(): the restatement's, and the counts that follow
    from the rule text alone."""
    same(got, saturated_tree_expectation(explore, playouts))
    v, w, l, a, nd, p = got.values()
    full = I_MAX * playouts
    other = saturated_boards()[3]
    assert v[0, WIN_ACTION] == I_MAX and w[0, WIN_ACTION] == full and l[0, WIN_ACTION] == 0 and a[0] == WIN_ACTION and nd[0] == 2 and p[0] == 0
    assert v[1, UNCOVER_ACTION] == I_MAX and l[1, UNCOVER_ACTION] == full and w[1, UNCOVER_ACTION] == 0 and a[1] == UNCOVER_ACTION and p[1] == 0
    assert v[2, WIN_ACTION] + v[2, other] == I_MAX and w[2, WIN_ACTION] == v[2, WIN_ACTION] * playouts and a[2] == WIN_ACTION
    assert v[2, other] >= 1 and v.sum() == 3 * I_MAX
    if explore == 0:  # (a decided win has the largest mean there is: without an exploration term the other child is visited once)
        assert v[2, other] == 1 and w[2, WIN_ACTION] == full - playouts


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


@pytest.mark.parametrize("explore", EXPLORES)
def test_tree_host_flavour_equals_restatement_at_the_largest_budget(cpu, explore):
    st, tm, mask, _ = saturated_boards()
    assert FULL == 1 << 18
    check_saturated_tree(run("tree_search", "cpu", st, tm, mask, (I_MAX, P_MAX, M_MAX, explore, SEED, ENV_BASE, CALL)), explore)


# gbl_collect_search takes no root mask, so its searches of these positions see every legal move, and a restatement of 1024 x 256
# games of up to 255 plies from open leaves is out of Python's reach.  With max_plies = 0 an open leaf's games all stay unfinished
# (nothing is played) while the decided leaves still count all 256 games of every visit: on the positions with the winning move the
# search piles nearly all of its 1024 visits and 2^18 games onto one child, which is what the int16 visits and the value sum have
# to hold.
COLLECT_EXPLORE = 0
_COLLECT = {}


def saturated_collect_args(sample_plies, layout="time"):
    st, tm, _, _ = saturated_boards()
    turn = np.zeros(3, np.int32)
    return (st, tm, turn, 1, ("tree", "tree"), (I_MAX, I_MAX), (P_MAX, P_MAX), 0, COLLECT_EXPLORE, sample_plies, nat.ILLEGAL_NOOP, layout, SEED,
            ENV_BASE, CALL)


def saturated_collect_expectation(sample_plies):
    if sample_plies not in _COLLECT:
        a = saturated_collect_args(sample_plies)
        _COLLECT[sample_plies] = restate_collect(*a[:11], *a[12:])
    return _COLLECT[sample_plies]


def check_saturated_collect(got, sample_plies):
    same_collect(got, saturated_collect_expectation(sample_plies))
    tr = got[0]
    v, value = tr["visits"][0].astype(np.int64), tr["value"][0]
    assert tr["visits"].dtype == np.int16 and (v.sum(1) == I_MAX).all() and (tr["nodes"][0] >= 2).all()
    # every root move but the best is tried once (54 actions at most), the rest of the 1024 visits are 256 won games each
    for b in (0, 2):
        assert v[b].max() >= I_MAX - 53 and value[b] >= (I_MAX - 53 - 53) * P_MAX and value[b] <= FULL
    assert (tr["how"][0] == (nat.HOW_SEARCH_SAMPLED if sample_plies else nat.HOW_SEARCH)).all()
    if not sample_plies:
        assert tr["actions"][0, 0] == tr["actions"][0, 2] and tr["winner"][0, 0] == 1 and tr["done"][0, 0] == 1  # the win is played
        assert tr["actions"][0, 1] != UNCOVER_ACTION


@pytest.mark.parametrize("sample_plies", [0, 1])
def test_collect_host_flavour_equals_restatement_at_the_largest_budget(cpu, sample_plies):
    for layout in ("time", "tile"):
        check_saturated_collect(collect(cpu, *saturated_collect_args(sample_plies, layout)), sample_plies)


# ---- "non-zero" means set: to_move and mask bytes other than 0 / 1 ----------------------------------------------------------------
def nonzero_bytes(x, seed):
    """x with every non-zero byte replaced by one of -128, -1, 2, 127."""
    rng = np.random.default_rng(seed)
    return np.where(x != 0, rng.choice(np.array([-128, -1, 2, 127], np.int8), x.shape), 0).astype(np.int8)


def byte_value_boards():
    """Six midgame boards, three per mover, a root mask of about half the actions, and the same inputs with other non-zero bytes."""
    from tests.test_playout_policy import random_midgames
    ms, mt = random_midgames(40, seed=12)
    pick = np.concatenate([np.flatnonzero(mt == 0)[:3], np.flatnonzero(mt == 1)[:3]])
    st, tm = ms[pick], mt[pick]
    mask = (np.random.default_rng(13).random((6, 54)) < 0.5).astype(np.int8)
    tm2, mask2 = nonzero_bytes(tm, 14), nonzero_bytes(mask, 15)
    assert tm.tolist() == [0, 0, 0, 1, 1, 1] and set(tm2[3:].tolist()) <= {-128, -1, 2, 127} and len(set(mask2.ravel().tolist())) == 5
    return st, tm, mask, tm2, mask2


TREE_BYTES = (24, 3, 20, 64, 5, 11, 2)  # iterations, playouts, max_plies, explore, seed, env_base, call
PLAYOUT_BYTES = (3, 20, 5, 11, 2)       # playouts, max_plies, seed, env_base, call


def test_nonzero_bytes_are_set_bytes(cpu):
    from tests import test_playout_policy as PP
    st, tm, mask, tm2, mask2 = byte_value_boards()
    exp = restate(st, tm, mask, *TREE_BYTES)
    for entry, exp, twin in (("tree_search", exp, restate(st, tm2, mask2, *TREE_BYTES)),
                             ("playout_values", PP.restate(st, tm, mask, *PLAYOUT_BYTES), PP.restate(st, tm2, mask2, *PLAYOUT_BYTES))):
        params = TREE_BYTES if entry == "tree_search" else PLAYOUT_BYTES
        for got in (run(entry, "cpu", st, tm, mask, params), run(entry, "cpu", st, tm2, mask2, params)):
            same(got, exp)
            same(got, twin)


# ---- the header's word on alignment ----------------------------------------------------------------------------------------------
def test_header_asks_no_alignment_of_the_search_inputs():
    """The 16-byte rule of the header's conventions is lifted for gbl_playout_values and gbl_tree_search in so many words (the
    GPU suite runs them on state / to_move / mask at odd addresses), and their "non-zero" reading of to_move and mask is stated."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(root, "include", "gobblet_hip.h")).read())
    for name in ("gbl_playout_values", "gbl_tree_search"):
        doc = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "need NO alignment" in doc and "4-byte aligned" in doc and "non-zero" in doc, name


# ---- the entry points' argument checks --------------------------------------------------------------------------------------------
def test_argument_errors_replay_the_recorded_table(golden_dir):
    """tests/golden/search_arg_errors.json: bad calls of gbl_playout_values, gbl_tree_search, gbl_collect_search and
    gbl_outcome_targets (every single violation, and double ones that pin which check fires first and which checks precede the
    n == 0 and plies == 0 returns) with the return code and the gbl_last_error text of either flavour, as recorded before the two
    flavours shared their checks.  Every call returns before any device work (the pointers are numbers, never read); a case whose
    "host" is null is an alignment rule, which only the device flavour has."""
    import json
    table = json.load(open(os.path.join(golden_dir, "search_arg_errors.json")))
    assert len(table) > 120 and {c["fn"] for c in table} == {"playout_values", "tree_search", "collect_search", "outcome_targets"}
    replay_arg_errors(table)
