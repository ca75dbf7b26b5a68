"""The root noise of gbl_tree_search_eval_noise / gbl_collect_search_noise restated in plain Python integers from the header text
alone (include/gobblet_hip.h, "Root noise"), for tests/test_root_noise.py and tests/test_gpu_root_noise.py.  The generator is the
oracle's Philox block, as tests/test_selfplay_search.py::word uses it; the search around the root row is
tests/evaluator_restatement.py's restate_search, imported and left as it is."""
import functools

import numpy as np

import oracle
from tests import evaluator_restatement as R

M32 = 0xFFFFFFFF
STREAM_NOISE = 6
T = (65536, 62757, 60097, 57549, 55109, 52773, 50535, 48393, 46341, 44376, 42495, 40693, 38968, 37316, 35734, 34219)


@functools.lru_cache(maxsize=64)
def _block(seed, g, counter, stream):
    return tuple(int(x) for x in oracle.philox4x32_10([g & M32, g >> 32, counter, stream], [seed & M32, seed >> 32]))


def word(seed, g, ply, stream):
    """The generator word of (seed, g, ply, stream): include/gobblet_hip.h, gbl_sample (one block serves four ply indices)."""
    return _block(seed, g, ply >> 2, stream)[ply & 3]


def noise_row(seed, g, q, cand):
    """nu: uint8[54] over the candidates cand (bool[54]); zeros where there is none."""
    nu = np.zeros(54, np.uint8)
    acts = [int(a) for a in np.flatnonzero(cand)]
    if not acts:
        return nu
    r = {a: word(seed, g, 64 * q + a, STREAM_NOISE) >> 24 for a in acts}
    low = min(r.values())
    e = {}
    for a in acts:
        d = r[a] - low
        assert 0 <= d <= 255
        e[a] = T[d & 15] >> (d >> 4)
    total = sum(e.values())
    for a in acts:
        nu[a] = 1 + (e[a] * 254) // total
    return nu


def mix(pi, nu, w, cand):
    """pi': uint8[54]."""
    out = np.zeros(54, np.uint8)
    for a in np.flatnonzero(cand):
        v = (int(pi[a]) * (256 - w) + int(nu[a]) * w + 128) >> 8
        assert 1 <= v <= 255
        out[a] = v
    return out


def restate_search_noise(net, state, to_move, mask, iterations, explore, w, seed, env_base, call):
    """gbl_tree_search_eval_noise: the seven outputs of restate_search (root_priors the network's row) and root_mixed.  The root
    node of restate_search keeps whatever is assigned to its `pi`: a root whose setter mixes the noise in is the whole substitution."""
    n = len(state)
    outs = []
    for b in range(n):
        g, mover = env_base + b, int(to_move[b] != 0)
        cand = R.candidates(state[b], mover, None if mask is None else mask[b])

        class RootMixingNode(R.Node):
            @property
            def pi(self):
                return self._pi

            @pi.setter
            def pi(self, row):
                if row is not None and self.parent is None and w > 0:
                    row = mix(row, noise_row(seed, g, call, cand), w, cand)
                self._pi = row

        plain = R.Node
        R.Node = RootMixingNode
        try:
            got = R.restate_search(net, state[b:b + 1], to_move[b:b + 1], None if mask is None else mask[b:b + 1], iterations, explore)
        finally:
            R.Node = plain
        mixed = got[6]
        pi = R.restate_evaluate(net, state[b:b + 1], to_move[b:b + 1], None if mask is None else mask[b:b + 1])[0]
        outs.append(got[:6] + (pi, mixed))
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(8))


def restate_collect_noise(st, tm, turn, T, pols, nets, its, deps, noise, X, sample_plies, illegal_mode, seed, env_base, ply0):
    """The contract of gbl_collect_search_noise, ply by ply, on the oracle: tests/test_selfplay_solve.py's restate_collect_solve with
    the search of ply q replaced by restate_search_noise(w = noise[mover], seed, g, call = q) over the same candidate set."""
    from gobblet_rl_amd import _native as nat
    from tests import solver_restatement as SR
    from tests.test_playout_policy import sample_stream
    from tests.test_selfplay_search import STREAM_VISIT, visits_draw
    from tests.test_selfplay_solve import NAMES, _solve_one
    n = len(st)
    st, tm, dn = st.copy(), tm.copy(), np.zeros(n, np.int8)
    turn = np.zeros(n, np.int32) if turn is None else turn.astype(np.int32).copy()
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
                if proven[b] != 0:  # no search, no draw
                    actions[b], how[b] = a_star, nat.HOW_PROVEN
                    visits[b, a_star] = its[m]
                    value[b] = (1 if proven[b] > 0 else -1) * 128 * its[m]
                    continue
                mask = (outcomes[b] == 0).astype(np.int8)[None]
            v, w, l, a, nd, rv, rp, _ = restate_search_noise(nets[m], st[b:b + 1], tm[b:b + 1], mask, its[m], X, noise[m], seed, g, q)
            visits[b], value[b], nodes[b], rootv[b], pri[b] = v[0], int((w[0] - l[0]).sum()), nd[0], rv[0], rp[0]
            if turn[b] < sample_plies:
                actions[b], how[b] = visits_draw(v[0], word(seed, g, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
            else:
                actions[b], how[b] = a[0], nat.HOW_SEARCH
        r = oracle.batch_step(st, tm, dn, actions, illegal_mode, auto_reset=True, turn=turn)
        for k, v in (("actions", actions), ("winner", r["winner"]), ("rewards", r["reward"]), ("done", dn.copy()), ("to_move", tm.copy()),
                     ("action_mask", r["mask"]), ("observation", r["obs"].reshape(n, 117)), ("visits", visits), ("value", value),
                     ("nodes", nodes), ("how", how), ("mover", mover), ("root_value", rootv), ("priors", pri), ("outcomes", outcomes),
                     ("proven", proven)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, st, tm, dn, turn
