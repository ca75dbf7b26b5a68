"""The Gumbel root rule of gbl_tree_search_gumbel / gbl_collect_search_gumbel restated in plain Python integers from the header text
alone (include/gobblet_hip.h, "Gumbel root search"), for tests/test_gumbel_search.py and tests/test_gpu_gumbel_search.py.  The generator
is the oracle's Philox block (tests/noise_restatement.py::word); the search below the root is tests/evaluator_restatement.py's
restate_search, imported and left as it is: its selection takes the candidate of the largest `key`, so a `key` that ranks the ROOT's
candidates by the rule (and halves before the first look of an iteration) is the whole substitution."""
import math

import numpy as np

import oracle
from tests import evaluator_restatement as R
from tests.noise_restatement import word

STREAM_GUMBEL = 10
HOW_GUMBEL = 10
GT = tuple(int(x) for x in np.rint(-np.log(-np.log((np.arange(256) + 0.5) / 256.0)) * 16.0 / math.log(2.0)))
NAMES = ("visits", "wins", "losses", "action", "nodes", "root_value", "root_priors", "target", "gumbel")


def gumbel_values(seed, g, q, cand, noise):
    """{a: g_a} over the candidates."""
    return {int(a): (GT[word(seed, g, 64 * q + int(a), STREAM_GUMBEL) >> 24] if noise else 0) for a in np.flatnonzero(cand)}


def root_logits(net, o, cand):
    """{a: L_a}: minus the distance below the largest logit over the candidates, capped at 255."""
    l = {int(a): int(o[a]) >> net.shift_p for a in np.flatnonzero(cand)}
    top = max(l.values())
    return {a: -min(top - x, 255) for a, x in l.items()}


def ceil_log2(m):
    p = 0
    while (1 << p) < m:
        p += 1
    return p


class Rule:
    """One root's rule: the considered set, the schedule, sigma, the decision and the target row."""

    def __init__(self, g, L, q_root, considered, iterations, visit_offset, scale):
        self.g, self.L, self.q_root, self.iterations, self.visit_offset, self.scale = g, L, q_root, iterations, visit_offset, scale
        m = min(considered, len(L))
        self.A = sorted(L, key=lambda a: (-(g[a] + L[a]), a))[:m]
        self.P = max(1, ceil_log2(m))
        self.T = max(1, iterations // (self.P * m))
        self.looked = -1  # the root's n at the last look: one halving check per iteration

    def sigma(self, root):
        """{a: sigma_a} over every candidate, now."""
        max_n = max((c.n for c in root.children.values()), default=0)
        out = {}
        for a in self.L:
            c = root.children.get(a)
            mean = ((c.W - c.L + c.n * R.P) << 15) // (c.n * R.P) if c is not None else 32768 + 256 * self.q_root
            assert 0 <= mean <= 65536
            prod = (self.visit_offset + max_n) * self.scale * mean
            assert prod < 1 << 32
            out[a] = prod >> 16
        return out

    def before_selection(self, root):
        if self.looked == root.n:
            return
        self.looked = root.n
        if len(self.A) > 2 and all(a in root.children and root.children[a].n >= self.T for a in self.A):
            s = self.sigma(root)
            keep = max(2, -(-len(self.A) // 2))
            self.A = sorted(self.A, key=lambda a: (-(self.g[a] + self.L[a] + s[a]), a))[:keep]
            self.T += max(1, self.iterations // (self.P * len(self.A)))

    def root_key(self, root, a):
        """What restate_search maximises at the root (ties to the lower action there): outside A below everything; inside A the fewest
        visits, then the larger g + L."""
        self.before_selection(root)
        if a not in self.A:
            return (0, 0, 0)
        c = root.children.get(a)
        return (1, -(c.n if c is not None else 0), self.g[a] + self.L[a])

    def decision(self, root):
        s = self.sigma(root)
        visits = lambda a: root.children[a].n if a in root.children else 0  # noqa: E731
        return min(self.A, key=lambda a: (-visits(a), -(self.g[a] + self.L[a] + s[a]), a))

    def target(self, root):
        s = self.sigma(root)
        t = {a: self.L[a] + s[a] for a in self.L}
        top = max(t.values())
        e = {}
        for a in t:
            d = min(top - t[a], 255)
            e[a] = R.T[d & 15] >> (d >> 4)
        total = sum(e.values())
        row = np.zeros(54, np.uint8)
        for a in t:
            row[a] = 1 + (e[a] * 254) // total
            assert 1 <= row[a] <= 255
        return row


def restate_search_gumbel(net, state, to_move, mask, iterations, explore, considered, noise, visit_offset, scale, seed, env_base, call):
    """gbl_tree_search_gumbel: the nine outputs in NAMES' order."""
    n = len(state)
    outs = []
    plain_key, plain_node = R.key, R.Node
    for b in range(n):
        mover = int(to_move[b] != 0)
        cand = R.candidates(state[b], mover, None if mask is None else mask[b])
        target, gum, rule, roots = np.zeros(54, np.uint8), np.zeros(54, np.int16), None, []
        if cand.any():
            o = R.outputs(net, state[b], mover)
            g = gumbel_values(seed, env_base + b, call, cand, noise)
            rule = Rule(g, root_logits(net, o, cand), R.value_of(net, o), considered, iterations, visit_offset, scale)
            for a, x in g.items():
                gum[a] = x

        class Keep(plain_node):  # (the root is the first node restate_search makes)
            def __init__(self, *args):
                super().__init__(*args)
                if self.parent is None:
                    roots.append(self)

        def key(v, a, x):
            return rule.root_key(v, a) if v.parent is None else (2, plain_key(v, a, x), 0)

        R.key, R.Node = key, Keep
        try:
            got = list(R.restate_search(net, state[b:b + 1], to_move[b:b + 1], None if mask is None else mask[b:b + 1], iterations, explore))
        finally:
            R.key, R.Node = plain_key, plain_node
        if rule is not None:
            got[3] = np.array([rule.decision(roots[0])], np.int32)
            target = rule.target(roots[0])
        outs.append(tuple(got) + (target[None], gum[None]))
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(9))


def restate_collect_gumbel(st, tm, turn, T, pols, nets, its, considered, noise, visit_offset, scale, X, sample_plies, illegal_mode, seed,
                           env_base, ply0):
    """The contract of gbl_collect_search_gumbel, ply by ply, on the oracle: a RANDOM side samples on stream 0; an EVAL_TREE side with
    considered 0 searches as in gbl_collect_search_eval (the stream-4 draw while turn < sample_plies); one with considered > 0 plays the
    rule's decision and leaves the target row in the visits' place.  Returns ({name: (T, n, ...)}, state, to_move, done, turn)."""
    from gobblet_rl_amd import _native as nat
    from tests.selfplay_harness import EVAL_NAMES
    from tests.test_playout_policy import sample_stream
    from tests.test_selfplay_search import STREAM_VISIT, visits_draw
    n = len(st)
    st, tm, dn = st.copy(), tm.copy(), np.zeros(n, np.int8)
    turn = np.zeros(n, np.int32) if turn is None else turn.astype(np.int32).copy()
    out = {k: [] for k, _, _ in EVAL_NAMES}
    for t in range(T):
        q = ply0 + t
        legal = oracle.batch_legal_mask(st, tm)
        actions, mover = np.zeros(n, np.int32), tm.copy()
        visits, value, nodes, how = np.zeros((n, 54), np.int16), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int8)
        rootv, pri = np.zeros(n, np.int32), np.zeros((n, 54), np.uint8)
        for b in range(n):
            m, g = int(tm[b]), env_base + b
            if pols[m] != "eval":
                actions[b] = sample_stream(legal[b], seed, g, q, 0)
                continue
            if considered[m] > 0:
                v, w, l, a, nd, rv, rp, tg, _ = restate_search_gumbel(nets[m], st[b:b + 1], tm[b:b + 1], None, its[m], X, considered[m], noise,
                                                                      visit_offset, scale, seed, g, q)
                visits[b], actions[b], how[b] = tg[0], a[0], HOW_GUMBEL
            else:
                v, w, l, a, nd, rv, rp = R.restate_search(nets[m], st[b:b + 1], tm[b:b + 1], None, its[m], X)
                visits[b] = v[0]
                if turn[b] < sample_plies:
                    actions[b], how[b] = visits_draw(v[0], word(seed, g, q, STREAM_VISIT)), nat.HOW_SEARCH_SAMPLED
                else:
                    actions[b], how[b] = a[0], nat.HOW_SEARCH
            value[b], nodes[b], rootv[b], pri[b] = int((w[0] - l[0]).sum()), nd[0], rv[0], rp[0]
        r = oracle.batch_step(st, tm, dn, actions, illegal_mode, auto_reset=True, turn=turn)
        for k, v in (("actions", actions), ("winner", r["winner"]), ("rewards", r["reward"]), ("done", dn.copy()), ("to_move", tm.copy()),
                     ("action_mask", r["mask"]), ("observation", r["obs"].reshape(n, 117)), ("visits", visits), ("value", value),
                     ("nodes", nodes), ("how", how), ("mover", mover), ("root_value", rootv), ("priors", pri)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}, st, tm, dn, turn
