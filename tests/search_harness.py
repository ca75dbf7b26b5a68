"""What the tests of the six single-decision entry points (gbl_playout_values, gbl_tree_search, gbl_evaluate, gbl_tree_search_eval,
gbl_tree_search_eval_noise, gbl_solve; either flavour) share: ONE table of their argument lists, one runner on host arrays and on the
device (every output filled with -7 / 99 and framed by canaries that are checked after the call), the comparison, the GPU modules'
fixtures, and the replayer of the recorded tests/golden/*_arg_errors.json tables.  A plain module: the fixtures are imported by name."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle

from gobblet_rl_amd import _native as nat

DEV = "cuda:0"
PAD = 16      # rows of -7 / 99 kept before and after every output on the device (16: the rows keep their 16-byte alignment)
GUARD = 0x5A  # the bytes around a misaligned buffer


def _out(name, dtype=np.int32, tail=()):
    return name, dtype, tail, 99 if dtype == np.uint8 else -7


_TREE = tuple(_out(k, tail=(54,)) for k in ("visits", "wins", "losses")) + (_out("action"), _out("nodes"))
_EVAL_TREE = _TREE + (_out("root_value"), _out("root_priors", np.uint8, (54,)))
# entry point -> (its scalar parameters, whether a gbl_evaluator follows the mask, its outputs (name, dtype, row tail, fill)), all in
# ABI order: (state, to_move, mask, [ev], scalars..., outputs..., n, stream)
ENTRIES = {
    "playout_values": (("playouts", "max_plies", "seed", "env_base", "call"), False,
                       (_out("wins", tail=(54,)), _out("losses", tail=(54,)), _out("action"), _out("plies"))),
    "tree_search": (("iterations", "playouts", "max_plies", "explore", "seed", "env_base", "call"), False, _TREE + (_out("plies"),)),
    "evaluate": ((), True, (_out("priors", np.uint8, (54,)), _out("value"), _out("logits", tail=(56,)))),
    "tree_search_eval": (("iterations", "explore"), True, _EVAL_TREE),
    "tree_search_eval_noise": (("iterations", "explore", "noise", "seed", "env_base", "call"), True,
                               _EVAL_TREE + (_out("root_mixed", np.uint8, (54,)),)),
    "solve": (("depth",), False, (_out("outcome", np.int8, (54,)), _out("value", np.int8), _out("action"))),
}
PLAYOUT_NAMES, TREE_NAMES, EVAL_NAMES, SEARCH_NAMES, NOISE_SEARCH_NAMES, SOLVE_NAMES = (
    tuple(o[0] for o in outs) for _, _, outs in ENTRIES.values())


class Call:
    """One entry point of one flavour on buffers of its own: load() the inputs (in place from the second time on: a captured launch
    holds the addresses), launch() on the current stream, results() -> {name: array} after checking every byte around the outputs
    and every input byte.  Outputs not in `keep` are NULL.  `net`: anything with struct() -> gbl_evaluator (a restatement Net on the
    host, a DeviceNet on the device).  misaligned: state / to_move / mask at odd addresses, every output at the least aligned
    address its type allows, GUARD bytes on either side."""

    def __init__(self, entry, device, net=None, keep=None, misaligned=False):
        self.scalars, self.takes_ev, self.outs = ENTRIES[entry]
        self.host, self.net, self.misaligned = device == "cpu", net, misaligned
        self.keep = [o[0] for o in self.outs] if keep is None else keep
        lib, prefix = (nat.cpu_raw(), "gbl_cpu_") if self.host else (nat.lib(), "gbl_")
        self.f, self.err = getattr(lib, prefix + entry), getattr(lib, prefix + "last_error")
        self.buf, self.frame = {}, {}

    def _put(self, key, a, lead, window=None):
        """`a` between `lead` and (misaligned) 256 GUARD bytes; window: (first byte, bytes, dtype, shape) of the rows inside `a`."""
        image = np.concatenate([np.full(lead, GUARD, np.uint8), a.reshape(-1).view(np.uint8), np.full(256 * self.misaligned, GUARD, np.uint8)])
        self.frame[key] = image, lead, window
        if self.host:
            self.buf[key] = image.copy()
        elif key in self.buf:
            import torch
            self.buf[key].copy_(torch.from_numpy(image))
        else:
            import torch
            self.buf[key] = torch.from_numpy(image).to(DEV)

    def load(self, st, tm, mask=None):
        self.n = len(st)
        for key, a, lead in (("state", st, 1), ("to_move", tm, 3), ("mask", mask, 5)):
            if a is not None:
                self._put(key, np.ascontiguousarray(a, np.int8), lead * self.misaligned)
        pad = 0 if self.host else PAD
        for key, dt, tail, fill in self.outs:
            if key in self.keep:
                rows = np.full((self.n + 2 * pad,) + tail, fill, dt)
                row = rows[0].nbytes
                self._put(key, rows, (8 - rows.itemsize) * self.misaligned, (pad * row, self.n * row, dt, (self.n,) + tail))
        return self

    def _ptr(self, key):
        if key not in self.frame:
            return None
        _, lead, window = self.frame[key]
        base = self.buf[key].ctypes.data if self.host else self.buf[key].data_ptr()
        return base + lead + (window[0] if window else 0)

    def launch(self, params=()):
        assert len(params) == len(self.scalars), self.scalars
        self.ev = self.net.struct() if self.takes_ev else None  # (alive until the call has returned)
        rc = self.f(*[self._ptr(k) for k in ("state", "to_move", "mask")], *([C.addressof(self.ev)] if self.takes_ev else []),
                    *[int(p) for p in params], *[self._ptr(o[0]) for o in self.outs], self.n, None if self.host else nat.current_stream(DEV))
        assert rc == 0, self.err()

    def results(self):
        got = {}
        for key, (image, lead, window) in self.frame.items():
            raw = self.buf[key] if self.host else self.buf[key].cpu().numpy()
            if window is None:
                assert np.array_equal(raw, image), "input %s was written" % key
                continue
            lo = lead + window[0]
            hi = lo + window[1]
            assert np.array_equal(raw[:lo], image[:lo]) and np.array_equal(raw[hi:], image[hi:]), "output %s was written outside its rows" % key
            got[key] = raw[lo:hi].copy().view(window[2]).reshape(window[3])
        return got


def run(entry, device, st, tm, mask, params, net=None, keep=None, misaligned=False):
    """gbl_<entry> on the device, or with device "cpu" gbl_cpu_<entry> on host arrays: {name: array} of the outputs in `keep` (None:
    all), in the table's order.  The device path synchronises once and copies back."""
    call = Call(entry, device, net, keep, misaligned).load(st, tm, mask)
    call.launch(params)
    if device != "cpu":
        import torch
        torch.cuda.synchronize()
    return call.results()


def same(got, exp):
    """Two {name: array} (or `exp` the arrays in the order of `got`): dtypes, then values; the first five differing indices."""
    if not isinstance(exp, dict):
        assert len(exp) == len(got)
        exp = dict(zip(got, exp))
    for k in got:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (k, np.argwhere(got[k] != exp[k])[:5])


# ---- fixtures of the GPU modules ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G():
    import torch

    import gobblet_rl_amd as g
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    g._native.lib()
    g._native.cpu_raw().gbl_cpu_set_threads(16)
    yield g
    g._native.cpu_raw().gbl_cpu_set_threads(0)


def midgame_boards(n=65536, device=DEV, turn=False, planted=False):
    """The positions of every search test: BatchedGobblet(n, seed=11).rollout(64), nobody holding a line (board b depends on b
    alone, so the first boards of a small environment are the first boards of the large one).  (state, to_move), with turn=True and
    their turn counters; planted: boards 1 and 2 are roots one move from a decided game."""
    import gobblet_rl_amd as g
    env = g.BatchedGobblet(n, device, auto_reset=True, seed=11, track_turn=turn)
    env.rollout(64)
    st, tm = env.squares.cpu().numpy().copy(), env.to_move.cpu().numpy().copy()
    assert (oracle.batch_winner(st) == 0).all() and (n < 65536 or 0.3 < tm.mean() < 0.7)
    if planted:
        from tests.solver_restatement import UNCOVER_SEQ, WIN_SEQ, play
        (st[1], tm[1]), (st[2], tm[2]) = play(WIN_SEQ), play(UNCOVER_SEQ)
    return (st, tm, env.turn.cpu().numpy().copy()) if turn else (st, tm)


# ---- the recorded argument errors --------------------------------------------------------------------------------------------------
def recorded_call(lib, prefix, case):
    """One case of a tests/golden/*_arg_errors.json table: every "ev" in its argument list is an evaluator, given as its eight fields
    (or null) in case["ev"] (one for the whole list) or case["evs"] (one after the other); a table without evaluators has neither.
    Every pointer is a number that is never read (all calls return before any work); where the ABI has a typed pointer (an int32_t *out)
    the number is cast to it.  Returns the return code."""
    evs = [None if e is None else nat.Evaluator(*e) for e in case.get("evs", [case.get("ev")])]
    it = iter(evs) if "evs" in case else itertools.repeat(evs[0])
    fn = getattr(lib, prefix + case["fn"])
    args = []
    for x, ctype in zip(case["args"], fn.argtypes):
        if x == "ev":
            e = next(it)
            x = None if e is None else C.addressof(e)
        elif isinstance(x, int) and isinstance(ctype, type) and issubclass(ctype, C._Pointer):
            x = C.cast(x, ctype)
        args.append(x)
    assert len(args) == len(case["args"]), case["fn"]
    return fn(*args)


def replay_arg_errors(table, flavours=("device", "host")):
    """Every case of such a table on the flavours named: the recorded return code and, for an error, the recorded message."""
    libs = {"device": (nat.lib, "gbl_"), "host": (nat.cpu_raw, "gbl_cpu_")}
    for c in table:
        for flavour in flavours:
            if c[flavour] is None:  # (an alignment rule: only the device flavour has it)
                continue
            lib, prefix = libs[flavour][0](), libs[flavour][1]
            rc, msg = c[flavour]
            assert recorded_call(lib, prefix, c) == rc, (flavour, c["fn"], c["case"])
            if rc:
                assert getattr(lib, prefix + "last_error")().decode() == msg, (flavour, c["fn"], c["case"])
