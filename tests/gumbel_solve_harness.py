"""What the tests of gbl_collect_gumbel_solve (either flavour) share, on top of tests/selfplay_harness.py, tests/gumbel_harness.py and
tests/test_selfplay_solve.py: the entry point's runner on host arrays and on the device (the family's geometry and canaries; the
argument list by name, ordered by nat.SELFPLAY_ARGS_MORE), the ply-by-ply loop on the host flavour's single-decision entry points with
the branches it met counted, the Python restatement of the rule, the cases of the issue and the census of the fixture's first ply by
gbl_cpu_solve.  A plain module: no fixtures."""
import ctypes as C
import functools

import numpy as np

import oracle

from gobblet_rl_amd import _native as nat
from gobblet_rl_amd._selfplay import TRAJ_BUFFERS
from tests import evaluator_restatement as R
from tests import gumbel_restatement as GR
from tests import solver_restatement as SR
from tests.gumbel_harness import GUMBEL_NAMES  # noqa: F401  (registers "tree_search_gumbel" with tests.search_harness.run)
from tests.search_harness import DEV, PAD, run
from tests.selfplay_harness import CODES, SOLVE_NAMES as NAMES, Compact, geometry
from tests.test_playout_policy import sample_stream
from tests.test_selfplay_search import STREAM_VISIT, visits_draw, word

ENTRY = "gbl_collect_gumbel_solve"
EXPLORE = 48
# (policies, considered, depths, iterations): the issue's four
CASES = ((("eval", "eval"), (16, 16), (2, 3), (16, 16)),
         (("eval", "eval"), (16, 0), (3, 3), (8, 16)),   # a Gumbel side against a guarded PUCT side
         (("eval", "eval"), (3, 54), (0, 2), (8, 12)),
         (("eval", "random"), (4, 4), (3, 0), (16, 16)))
# gbl_cpu_solve of the fixture's first ply, boards x depth -> (proven wins, proven losses, unproven, unproven with a proven-loss action
# removed, unproven with |C| < 16), as the issue's table has them
CENSUS = {(65, 2): (30, 3, 32, 10, 7), (65, 3): (35, 3, 27, 9, 7), (130, 2): (60, 4, 66, 20, 17), (130, 3): (68, 4, 58, 17, 15)}
SMALLEST_C = {65: 3, 130: 2}
BRANCHES = ("proven win", "proven loss", "rule over the legal set", "rule over a strict subset", "rule with |C| < considered",
            "keys over C", "unguarded rule", "random")


def census(st, tm, depth):
    """The first ply's branches by the solver alone: CENSUS's five numbers, and the smallest |C| of an unproven root."""
    outcome, V, _ = run("solve", "cpu", st, tm, None, (depth,)).values()
    unproven = V == 0
    size = (outcome[unproven] == 0).sum(1)
    removed = ((outcome[unproven] < 0) & (outcome[unproven] != SR.NONE)).any(1)
    return ((V > 0).sum(), (V < 0).sum(), unproven.sum(), removed.sum(), (size < 16).sum()), size.min()


def call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, X, sample_plies, illegal_mode, counters, tn, stream, evs,
              its, deps, considered, gumbel_noise, visit_offset, scale):
    ev0, ev1 = (None if e is None else C.addressof(e) for e in evs)
    every = dict(state=ptr(st), to_move=ptr(tm), done=ptr(dn), **{arg: ptr(traj.get(k)) for arg, k in TRAJ_BUFFERS.items()}, n=n,
                 ply_stride=ps, tile_stride=ts, seed=seed, env_base=env_base, ply0=ply0, ply_dev=ptr(pd), plies=T, policy0=CODES[pols[0]],
                 policy1=CODES[pols[1]], ev0=ev0, ev1=ev1, iterations0=its[0], iterations1=its[1], solve_depth0=deps[0], solve_depth1=deps[1],
                 explore=X, sample_plies=sample_plies, illegal_mode=illegal_mode, counters=ptr(counters), turn=ptr(tn),
                 considered0=int(considered[0]), considered1=int(considered[1]), gumbel_noise=int(gumbel_noise), visit_offset=int(visit_offset),
                 scale=int(scale), stream=stream)
    return nat.selfplay_args(ENTRY, **{k: every[k] for k, _ in nat.SELFPLAY_ARGS_MORE[ENTRY]})


def _run(f, ok, put, get, ptr, pad, stream, st, tm, turn, T, pols, nets, its, deps, considered, noise, visit_offset, scale, X, sample_plies,
         illegal_mode, layout, seed, env_base, ply0, ply_dev=None, keep=None, counters=None, odd=()):
    """tests.selfplay_harness._run for this entry point.  odd: outputs (of one-byte cells) handed over from an odd address."""
    n = len(st)
    ps, ts, total, at = geometry(n, T, layout)
    store = Compact(put, get, pad)
    keep = [k for k, _, _ in NAMES] if keep is None else keep
    traj = {}
    for k, dt, tail in NAMES:
        if k not in keep:
            continue
        if k in odd:  # one spare byte in front: the cells start at an odd address, the canaries go with them
            cell = int(np.prod(tail, dtype=np.int64))
            flat = put(np.full(1 + (total + 2 * pad) * cell, -7, np.int8))
            store.full[k] = flat[1:].reshape((total + 2 * pad,) + tail)
            traj[k] = store.full[k][pad:]
            assert ptr(traj[k]) % 2 == 1
        else:
            traj[k] = store.array(k, dt, tail, total)
    st, tm, dn = put(np.ascontiguousarray(st, np.int8)), put(np.ascontiguousarray(tm, np.int8)), put(np.full(n, 5, np.int8))
    tn = None if turn is None else put(np.ascontiguousarray(turn, np.int32))
    pd = None if ply_dev is None else put(np.array([ply_dev], np.int32))
    evs = [None if net is None else net.struct() for net in nets]  # (alive until the call has returned)
    ok(f(*call_args(ptr, st, tm, dn, traj, n, ps, ts, seed, env_base, ply0, pd, T, pols, X, sample_plies, illegal_mode, counters, tn, stream,
                    evs, its, deps, considered, noise, visit_offset, scale)))
    return store.cells(at, total), get(st), get(tm), get(dn), None if tn is None else get(tn)


def host_collect_gs(st, tm, turn, T, pols, nets, its, deps, considered, noise=1, visit_offset=50, scale=23, X=EXPLORE, sample_plies=0,
                    illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, **kw):
    """gbl_cpu_collect_gumbel_solve on host arrays; nets: restatement Nets (None for a RANDOM side); kw: ply_dev=, keep=, counters=.
    Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    L = nat.cpu_raw()

    def ok(rc):
        assert rc == 0, L.gbl_cpu_last_error()
    return _run(L.gbl_cpu_collect_gumbel_solve, ok, np.array, lambda a: a, lambda a: None if a is None else a.ctypes.data, 0, None, st, tm,
                turn, T, pols, nets, its, deps, considered, noise, visit_offset, scale, X, sample_plies, illegal_mode, layout, seed, env_base,
                ply0, **kw)


def device_collect_gs(st, tm, turn, T, pols, nets, its, deps, considered, noise=1, visit_offset=50, scale=23, X=EXPLORE, sample_plies=0,
                      illegal_mode=nat.ILLEGAL_NOOP, layout="time", seed=1, env_base=0, ply0=0, **kw):
    """gbl_collect_gumbel_solve on the device, every output between canaries; nets: DeviceNets; kw as host_collect_gs, and odd=."""
    import torch

    def get(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()
    return _run(nat.lib().gbl_collect_gumbel_solve, lambda rc: nat.check(rc, ENTRY), lambda a: torch.from_numpy(a).to(DEV), get, nat.ptr, PAD,
                nat.current_stream(DEV), st, tm, turn, T, pols, nets, its, deps, considered, noise, visit_offset, scale, X, sample_plies,
                illegal_mode, layout, seed, env_base, ply0, **kw)


def composed_loop(cpu, st, tm, turn, T_, pols, nets, its, deps, considered, noise, vo, scale, X, sample_plies, illegal_mode, seed, env_base,
                  ply0):
    """The rule, ply by ply, on the host flavour's own single-decision entry points: gbl_cpu_solve -> the proven pick, or
    gbl_cpu_tree_search_gumbel(mask = C, call = q) / gbl_cpu_tree_search_eval(mask = C) -> gbl_cpu_step_into.  A side's boards go
    through an entry point together, every other row under an empty mask, so that the call's env_base + b is the board's id.
    Returns (the 16 arrays (T, n, ...), state, to_move, done, turn, {branch: plies that took it})."""
    n = len(st)
    s, m, d, tn = st.copy(), tm.copy(), np.zeros(n, np.int8), turn.astype(np.int32).copy()
    plies, met = [], dict.fromkeys(BRANCHES, 0)
    for t in range(T_):
        q = ply0 + t
        act, vis, val, nod = np.zeros(n, np.int32), np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32)
        rv, pri, how = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8), np.zeros(n, np.int8)
        outcomes, proven = np.full((n, 54), SR.NONE, np.int8), np.zeros(n, np.int8)
        legal = oracle.batch_legal_mask(s, m).astype(np.int8)
        for side in (0, 1):
            mine = (m == side) & legal.any(1)
            if pols[side] != "eval":
                for b in np.flatnonzero(m == side):
                    act[b] = sample_stream(legal[b], seed, env_base + int(b), q, 0)
                met["random"] += int((m == side).sum())
                continue
            if not mine.any():
                continue
            cand = legal * mine[:, None]  # the candidates of this side's search: C under the guard, the legal mask without it
            if deps[side] > 0:
                outcome, V, a_star = run("solve", "cpu", s, m, cand, (deps[side],)).values()
                outcomes[mine], proven[mine] = outcome[mine], V[mine]
                won, lost = mine & (V > 0), mine & (V < 0)
                for rows, sign in ((won, 1), (lost, -1)):
                    idx = np.flatnonzero(rows)
                    act[idx], how[idx], val[idx] = a_star[idx], nat.HOW_PROVEN, sign * 128 * its[side]
                    vis[idx, a_star[idx]] = its[side]
                met["proven win"] += int(won.sum())
                met["proven loss"] += int(lost.sum())
                mine = mine & (V == 0)
                cand = ((outcome == 0) & mine[:, None]).astype(np.int8)
                assert cand[mine].any(1).all()
            idx = np.flatnonzero(mine)
            if not len(idx):
                continue
            size = cand[idx].sum(1)
            if considered[side] > 0:
                o = run("tree_search_gumbel", "cpu", s, m, cand, (its[side], X, considered[side], noise, vo, scale, seed, env_base, q),
                        nets[side])
                vis[idx], act[idx], how[idx] = o["target"][idx], o["action"][idx], nat.HOW_GUMBEL
                if deps[side] > 0:
                    whole = size == legal[idx].sum(1)
                    met["rule over the legal set"] += int(whole.sum())
                    met["rule over a strict subset"] += int((~whole).sum())
                    met["rule with |C| < considered"] += int((size < considered[side]).sum())
                else:
                    met["unguarded rule"] += len(idx)
            else:
                o = run("tree_search_eval", "cpu", s, m, cand, (its[side], X), nets[side])
                vis[idx] = o["visits"][idx]
                for b in idx:
                    if tn[b] < sample_plies:
                        act[b], how[b] = visits_draw(o["visits"][b], word(seed, env_base + int(b), q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
                    else:
                        act[b], how[b] = o["action"][b], nat.HOW_SEARCH
                met["keys over C"] += len(idx)
            val[idx], nod[idx], rv[idx], pri[idx] = (o["wins"][idx] - o["losses"][idx]).sum(1), o["nodes"][idx], o["root_value"][idx], \
                o["root_priors"][idx]
        mover = m.copy()
        win, rew = np.zeros(n, np.int8), np.zeros((n, 2), np.int8)
        mask_, obs = np.zeros((n, 54), np.int8), np.zeros((n, 117), np.int8)
        rc = cpu.gbl_cpu_step_into(s.ctypes.data, m.ctypes.data, d.ctypes.data, act.ctypes.data, win.ctypes.data, rew.ctypes.data,
                                   mask_.ctypes.data, obs.ctypes.data, tn.ctypes.data, None, None, None, n, illegal_mode, 1, None)
        assert rc == 0, cpu.gbl_cpu_last_error()
        plies.append(dict(actions=act, winner=win, rewards=rew, done=d.copy(), to_move=m.copy(), action_mask=mask_, observation=obs,
                          visits=vis, value=val, nodes=nod, how=how, mover=mover, root_value=rv, priors=pri, outcomes=outcomes, proven=proven))
    return {k: np.stack([p[k] for p in plies]) for k in plies[0]}, s, m, d, tn, met


@functools.lru_cache(maxsize=None)
def _solve_one(state_bytes, mover, depth):
    o, v, a = SR.solve(np.frombuffer(state_bytes, np.int8)[None], np.array([mover], np.int8), None, depth)
    return o[0], int(v[0]), int(a[0])


def restate_collect_gs(st, tm, turn, T, pols, nets, its, deps, considered, noise, visit_offset, scale, X, sample_plies, illegal_mode, seed,
                       env_base, ply0):
    """The rule's text once more in Python, ply by ply, on the oracle: tests/solver_restatement.py decides what is proven,
    tests/gumbel_restatement.py (considered > 0) or tests/evaluator_restatement.py (considered 0) searches C, the oracle steps."""
    n = len(st)
    st, tm, dn = st.copy(), tm.copy(), np.zeros(n, np.int8)
    turn = turn.astype(np.int32).copy()
    out = {k: [] for k, _, _ in NAMES}
    for t in range(T):
        q = ply0 + t
        legal = oracle.batch_legal_mask(st, tm)
        actions, mover = np.zeros(n, np.int32), tm.copy()
        visits, value, nodes, how = np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int8)
        rootv, pri = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8)
        outcomes, proven = np.full((n, 54), SR.NONE, np.int8), np.zeros(n, np.int8)
        for b in range(n):
            m, g = int(tm[b]), env_base + b
            if pols[m] != "eval":
                actions[b] = sample_stream(legal[b], seed, g, q, 0)
                continue
            mask = None
            if deps[m] > 0 and legal[b].any():
                outcomes[b], proven[b], a_star = _solve_one(st[b].tobytes(), m, deps[m])
                if proven[b] != 0:
                    actions[b], how[b] = a_star, nat.HOW_PROVEN
                    visits[b, a_star] = its[m]
                    value[b] = (1 if proven[b] > 0 else -1) * 128 * its[m]
                    continue
                mask = (outcomes[b] == 0).astype(np.int8)[None]
            if considered[m] > 0:
                v, w, l, a, nd, rv, rp, tg, _ = GR.restate_search_gumbel(nets[m], st[b:b + 1], tm[b:b + 1], mask, its[m], X, considered[m],
                                                                         noise, visit_offset, scale, seed, g, q)
                visits[b], actions[b], how[b] = tg[0], a[0], nat.HOW_GUMBEL
            else:
                v, w, l, a, nd, rv, rp = R.restate_search(nets[m], st[b:b + 1], tm[b:b + 1], mask, its[m], X)
                visits[b] = v[0]
                if turn[b] < sample_plies:
                    actions[b], how[b] = visits_draw(v[0], word(seed, g, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
                else:
                    actions[b], how[b] = a[0], nat.HOW_SEARCH
            value[b], nodes[b], rootv[b], pri[b] = int((w[0] - l[0]).sum()), nd[0], rv[0], rp[0]
        r = oracle.batch_step(st, tm, dn, actions, illegal_mode, auto_reset=True, turn=turn)
        for k, v in (("actions", actions), ("winner", r["winner"]), ("rewards", r["reward"]), ("done", dn.copy()), ("to_move", tm.copy()),
                     ("action_mask", r["mask"]), ("observation", r["obs"].reshape(n, 117)), ("visits", visits), ("value", value),
                     ("nodes", nodes), ("how", how), ("mover", mover), ("root_value", rootv), ("priors", pri), ("outcomes", outcomes),
                     ("proven", proven)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, st, tm, dn, turn
