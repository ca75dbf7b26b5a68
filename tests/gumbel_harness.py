"""What the tests of gbl_tree_search_gumbel and gbl_collect_search_gumbel (either flavour) share, on top of tests/search_harness.py and
tests/selfplay_harness.py: the single-decision entry point's line in the harness's table (so that `run` serves it, canaries and all),
the self-play runner calls under the rule's own argument order and defaults (tests/selfplay_harness.py's one runner serves the entry
point as "gumbel"), and the boards.  A plain module: no fixtures."""
import math

import numpy as np
import torch

import oracle

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import evaluator_restatement as R
from tests import search_harness as SH
from tests import solver_restatement as SR
from tests.selfplay_harness import device_collect, host_collect

SH.ENTRIES.setdefault("tree_search_gumbel", (
    ("iterations", "explore", "considered", "gumbel_noise", "visit_offset", "scale", "seed", "env_base", "call"), True,
    SH._EVAL_TREE + (SH._out("target", np.uint8, (54,)), SH._out("gumbel", np.int16, (54,)))))
GUMBEL_NAMES = tuple(o[0] for o in SH.ENTRIES["tree_search_gumbel"][2])

PAIRS = ((1, 8), (2, 8), (3, 8), (4, 16), (5, 12), (16, 16), (16, 64), (54, 16))  # (considered, iterations)
# the long schedules: 54 -> 27 -> 14 -> 7 -> 4 -> 2, 27 -> 14 -> 7 -> 4 -> 2, 32 -> 16 -> 8 -> 4 -> 2 and 7 -> 4 -> 2 (a first target above 1)
LONG_PAIRS = ((54, 512), (27, 200), (32, 256), (7, 96))


def rule_boards(midgames):
    """The roots of the rule's tests from (state, to_move) midgames: two empty boards (54 candidates, either mover), the midgames, and
    eight more rows under masks that keep 27, 2, 1 and 0 candidates of an empty board and of a midgame.  Returns (state, to_move,
    mask, {candidates: a board that has so many})."""
    ms, mt = midgames
    st = np.concatenate([np.zeros((2, 27), np.int8), ms, np.zeros((4, 27), np.int8), ms[:4]])
    tm = np.concatenate([np.array([0, 1], np.int8), mt, np.array([0, 1, 0, 1], np.int8), mt[:4]])
    mask = np.ones((len(st), 54), np.int8)
    first, where = 2 + len(ms), {54: 0}
    for i, keep in enumerate((27, 2, 1, 0, 27, 2, 1, 0)):
        b = first + i
        legal = np.flatnonzero(oracle.legal_mask(st[b], int(tm[b])))
        assert len(legal) >= keep
        mask[b] = 0
        mask[b, legal[::-1][:keep]] = 1  # (the highest actions: the lowest-action tie-break has something to do)
        where.setdefault(keep, b)
    return np.ascontiguousarray(st), np.ascontiguousarray(tm), mask, where


# ---- the rule's arithmetic edges: one case each for either flavour ----------------------------------------------------------------------
# A builder returns ((state, to_move), mask, net, params, expect): `params` in the order of ENTRIES["tree_search_gumbel"], `expect(got)`
# asserts the closed-form expectation on the outputs `got` of run("tree_search_gumbel", ..., params, net) -- of the host flavour in
# tests/test_gumbel_search.py, of the kernel in tests/test_gpu_gumbel_long.py.
EDGE_EXPLORE = 48


def exact_target(L, sigma):
    """The header's sentence on the target row once more in exact integers, from {a: L_a} and {a: sigma_a}."""
    t = {a: L[a] + sigma[a] for a in L}
    top = max(t.values())
    e = {}
    for a in t:
        d = min(top - t[a], 255)
        e[a] = int(math.floor(65536 * 2.0 ** (-(d % 16) / 16) + 0.5)) // (2 ** (d // 16))
    row = np.zeros(54, np.uint8)
    for a in t:
        row[a] = 1 + (254 * e[a]) // sum(e.values())
    return row


def sigma_edge_case():
    """visit_offset 255, scale 64, 512 iterations under one considered action that wins at once: (255 + 512) * 64 * 65536 = 3 217 031 168,
    above 2^31 and below 2^32; sigma = 49 088, every other action lies more than 255 below and keeps the floor byte."""
    s, m = SR.play(SR.WIN_SEQ)
    logits = np.zeros(54, np.int64)
    logits[SR.WIN_ACTION] = 9

    def expect(got):
        assert got["visits"][0, SR.WIN_ACTION] == 512 and got["wins"][0, SR.WIN_ACTION] == 512 * 128 and got["action"][0] == SR.WIN_ACTION
        legal = np.flatnonzero(oracle.legal_mask(s, m))
        sigma = {int(a): (767 * 64 * 32768) >> 16 for a in legal}
        sigma[SR.WIN_ACTION] = (767 * 64 * 65536) >> 16
        assert sigma[SR.WIN_ACTION] == 49088 and 767 * 64 * 65536 >= 1 << 31
        row = exact_target({int(a): int(logits[a]) - 9 for a in legal}, sigma)
        assert np.array_equal(got["target"][0], row) and row[SR.WIN_ACTION] == 254 and (row[legal] >= 1).all()
        assert (np.delete(row[legal], np.flatnonzero(legal == SR.WIN_ACTION)) == 1).all()  # (the floor byte)
    return (s[None], np.array([m], np.int8)), None, R.logit_dial(logits), (512, EDGE_EXPLORE, 1, 0, 255, 64, 0, 0, 0), expect


def root_value_edge_case(q_raw, visit_offset, scale):
    """considered = 1 on the empty board: one child is visited, 53 actions go through the root's q.  The visited child's mean comes from
    the raw wins / losses / visits the entry point writes, by the header's formula."""
    logits = -(np.arange(54) % 7).astype(np.int64) * 5
    net = R.logit_dial(logits + 100, o54=q_raw << 2, shift_v=2)

    def expect(got):
        assert got["root_value"][0] == q_raw and got["visits"][0, 0] == 6 and got["visits"][0].sum() == 6
        W, Lo = int(got["wins"][0, 0]), int(got["losses"][0, 0])
        mean = {a: 32768 + 256 * q_raw for a in range(54)}
        mean[0] = ((W - Lo + 6 * 128) << 15) // (6 * 128)
        sigma = {a: ((visit_offset + 6) * scale * mean[a]) >> 16 for a in range(54)}
        assert np.array_equal(got["target"][0], exact_target({a: int(logits[a]) for a in range(54)}, sigma)), (visit_offset, scale)
    return (np.zeros((1, 27), np.int8), np.zeros(1, np.int8)), None, net, (6, EDGE_EXPLORE, 1, 0, visit_offset, scale, 0, 0, 0), expect


def winning_action_case(seed, env_base, n=512):
    """Flat logits and value 0: every leaf's mean is 32768 but a won child's 65536, so sigma lifts an action that wins at once over every
    Gumbel value ((50 + maxN) * 23 / 2 > 575, the g's span 186).  The position has four such actions (any piece onto square 2); one is
    in A iff its g is among the 16 largest (the lower action on ties).  A winner is decided whenever one is considered, the considered
    winners -- and nobody else -- carry the largest target byte, and a winner outside A goes through the root's value like the rest."""
    s, m = SR.play(SR.WIN_SEQ)

    def expect(got):
        legal = np.flatnonzero(oracle.legal_mask(s, m)).tolist()
        mine = 1 if m == 0 else -1
        winners = {a for a in legal if oracle.check_for_winner(oracle.play_turn(s, m, a)) == mine}
        assert SR.WIN_ACTION in winners and len(winners) == 4
        g = G.gumbel_row(seed, env_base + torch.arange(n), 3).numpy().astype(np.int64)
        some = 0
        for b in range(n):
            considered = winners & set(sorted(legal, key=lambda a: (-g[b, a], a))[:16])
            assert (int(got["action"][b]) in winners) == bool(considered), b
            if considered:
                some += 1
                row = got["target"][b]
                assert int(got["action"][b]) in considered and set(np.flatnonzero(row == row.max()).tolist()) == considered
                assert all(got["wins"][b, a] == 128 * got["visits"][b, a] > 0 for a in considered)
        assert n // 10 < some < n - n // 10  # (both cases occur)
    return (np.repeat(s[None], n, 0), np.full(n, m, np.int8)), None, R.zero_net(64), (16, EDGE_EXPLORE, 16, 1, 50, 23, seed, env_base, 3), expect


def host_collect_gumbel(st, tm, turn, T, pols, nets, its, considered, noise=1, visit_offset=50, scale=23, X=16, sample_plies=0,
                        illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, **kw):
    """gbl_cpu_collect_search_gumbel on host arrays (tests.selfplay_harness's one runner, as "gumbel", under the rule's own argument order
    and defaults); nets: restatement Nets; kw: ply_dev=, keep=, counters=, strides=, store=.  Returns ({name: (T, n, ...)}, state,
    to_move, done, turn)."""
    L = nat.cpu_raw()
    return host_collect("gumbel", L.gbl_cpu_collect_search_gumbel, L.gbl_cpu_last_error, st, tm, turn, T, pols, X, sample_plies, illegal_mode,
                        layout, seed, env_base, ply0, nets=nets, its=its, considered=considered, gumbel_noise=noise, visit_offset=visit_offset,
                        scale=scale, **kw)


def device_collect_gumbel(st, tm, turn, T, pols, nets, its, considered, noise=1, visit_offset=50, scale=23, X=16, sample_plies=0,
                          illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, **kw):
    """gbl_collect_search_gumbel on the device, every output between canaries; nets: DeviceNets."""
    return device_collect("gumbel", st, tm, turn, T, pols, X, sample_plies, illegal_mode, layout, seed, env_base, ply0, nets=nets, its=its,
                          considered=considered, gumbel_noise=noise, visit_offset=visit_offset, scale=scale, **kw)
