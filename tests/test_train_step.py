"""gbl_train_step, host flavour (no GPU): gbl_cpu_train_step against the numpy-float32 restatement of the header's bit-defined rule
(tests/train_restatement.py) bit for bit, its edges, its gradient against float64 autograd with torch's own float32 autograd as the
yardstick, its Adam update against the float64 formula, the error of its polynomial exp and log, a fit that learns and quantises,
and the argument errors."""
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import train_restatement as R
from tests.search_harness import replay_arg_errors
from tests.test_evaluator_edges import compare_with_float, open_positions  # noqa: F401  (a helper and a fixture, reused as they are)

F = np.float32
SHAPES = [(b, h) for b in (1, 3, 65, 130) for h in (64, 256)]   # (130 rows: chunks of 64, 64 and 2; 65: 64 and 1)


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


def fresh(hidden, seed=None):
    p = R.init_params(hidden, hidden if seed is None else seed)
    return p, np.zeros_like(p), np.zeros_like(p)


# ---- 1. bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", SHAPES)
@pytest.mark.parametrize("with_mask", [True, False])
def test_bits_equal_the_restatement(cpu, B, H, with_mask):
    """One step, and five consecutive steps (the moments and the bias corrections move), every output."""
    obs, mask, visits, z = R.random_batch(B, 7 * B + H, with_mask)
    assert 130 // R.CHUNK == 2 and 130 % R.CHUNK  # (the largest batch straddles the chunk size)
    p, m, v = fresh(H)
    for t in range(1, 6):
        hy = R.hyper_at(t)
        got = R.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy)
        R.same_bits(got, R.restate_step(obs, mask, visits, z, H, p, m, v, hy), (B, H, with_mask, t))
        assert got[4][2] == (B if B < 4 else B - 2) and np.isfinite(got[4]).all()
        if t == 1:
            no_grad = R.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, grad=False)   # grad_out is optional
            R.same_bits(no_grad, got, "grad_out NULL")
        p, m, v = got[:3]
        obs, mask, visits, z = R.random_batch(B, 7 * B + H + t, with_mask)   # (a fresh batch per step)


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------------
def test_a_batch_without_a_counted_row(cpu):
    obs, mask, visits, z, _, p, _ = R.EDGES["none counted"]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    assert (z[[0, 1, 2, 4]] == R.Z_OPEN).all() and z[3] == 1 and not visits[3].any()
    got = R.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy)
    assert np.array_equal(got[3], hy["weight_decay"] * p) and np.array_equal(got[4], np.zeros(4, F))
    assert all(np.isfinite(a).all() for a in got)
    R.same_bits(got, R.restate_step(obs, mask, visits, z, 64, p, m, v, hy))


def test_open_rows_among_counted_ones_add_nothing(cpu):
    obs, mask, visits, z, _, p, _ = R.EDGES["open rows"]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    got = R.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy)
    assert got[4][2] == 40 - 2 - 3
    R.same_bits(got, R.restate_step(obs, mask, visits, z, 64, p, m, v, hy))
    rng = np.random.default_rng(0)
    for r in (1, 2, 5, 17, 39):                 # whatever an uncounted row holds (row 2: only outside its visits) changes nothing
        obs[r] = rng.integers(0, 2, 117)
        if r != 2:
            visits[r] = rng.integers(0, 99, 54)
    R.same_bits(R.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy), got, "uncounted rows rewritten")


def test_a_row_with_one_candidate(cpu):
    obs, mask, visits, z, _, p, _ = R.EDGES["one candidate"]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    assert (mask != 0).sum() == 1
    got = R.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy)
    R.same_bits(got, R.restate_step(obs, mask, visits, z, 64, p, m, v, hy))
    rows = R.restate_rows(obs, mask, visits, z, 64, p, hy["value_reg"])
    assert got[4][0] == 0.0 and not rows["do"][0, :54].any() and rows["do"][0, 54] != 0     # p = 1: no policy loss, no policy gradient
    g_w2, g_b2 = R.split(got[3], 64)[2:]
    decay = R.split(hy["weight_decay"] * p, 64)
    assert np.array_equal(g_w2[:, :54], decay[2][:, :54]) and np.array_equal(g_b2[:54], decay[3][:54])
    assert not np.array_equal(g_w2[:, 54], decay[2][:, 54])


def test_logits_200_apart(cpu):
    """exp underflows to 0 under the max-subtracted form; the loss stays finite through the log-sum form."""
    obs, _, visits, z, _, p, _ = R.EDGES["logits 200 apart"]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    rows = R.restate_rows(obs, None, visits, z, 64, p, hy["value_reg"])
    assert (rows["o"][:, 0] - rows["o"][:, 1] == 200).all() and (R.exp32(rows["o"][:, :54] - rows["o"][:, :1])[:, 1] == 0).all()
    got = R.run_step(cpu, obs, None, visits, z, 64, p, m, v, hy)
    R.same_bits(got, R.restate_step(obs, None, visits, z, 64, p, m, v, hy))
    assert all(np.isfinite(a).all() for a in got) and 199.9 < got[4][0] < 200.5


@pytest.mark.parametrize("value", R.VALUES)
def test_value_column_below_at_and_above_one(cpu, value):
    obs, mask, visits, z, _, p, _ = R.EDGES["value %g" % value]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    rows = R.restate_rows(obs, mask, visits, z, 64, p, hy["value_reg"])
    assert rows["o"][0, 54] == F(value)
    got = R.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy)
    R.same_bits(got, R.restate_step(obs, mask, visits, z, 64, p, m, v, hy))
    inside = -1 < value < 1
    do54 = F(2) * (F(value) - F(1) if inside else F(0)) + F(2) * (hy["value_reg"] * F(value))     # no gradient through the clamp at or beyond 1
    assert R.split(got[3], 64)[3][54] == do54 / F(1) + hy["weight_decay"] * F(value)
    clipped = F(min(max(value, -1.0), 1.0))
    assert got[4][1] == (clipped - F(1)) * (clipped - F(1)) + hy["value_reg"] * (F(value) * F(value))


def test_a_hidden_unit_at_exactly_zero(cpu):
    obs, mask, visits, z, _, p, _ = R.EDGES["hidden unit at 0"]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    w2 = R.split(p, 64)[2]
    rows = R.restate_rows(obs, mask, visits, z, 64, p, hy["value_reg"])
    assert (rows["pre"][:, 7] == 0).all() and (rows["pre"][:, 8] > 0).any()
    got = R.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy)
    R.same_bits(got, R.restate_step(obs, mask, visits, z, 64, p, m, v, hy))
    g_w1, g_b1, g_w2, _ = R.split(got[3], 64)
    assert not g_w1[:, 7].any() and g_b1[7] == 0 and np.array_equal(g_w2[7], hy["weight_decay"] * w2[7])   # relu' is 0 at 0


@pytest.mark.parametrize("edge", ["weight_decay 0", "value_reg 0", "both 0"])
def test_weight_decay_and_value_reg_of_zero(cpu, edge):
    obs, mask, visits, z, _, p, off = R.EDGES[edge]()
    m, v = np.zeros_like(p), np.zeros_like(p)
    assert off and not any(off.values())
    for t in (1, 2):
        hy = R.hyper_at(t, **off)
        got = R.run_step(cpu, obs, mask, visits, z, 128, p, m, v, hy)
        R.same_bits(got, R.restate_step(obs, mask, visits, z, 128, p, m, v, hy), (off, t))
        p, m, v = got[:3]
    if "weight_decay" in off:
        z[:] = R.Z_OPEN
        got = R.run_step(cpu, obs, mask, visits, z, 128, p, m, v, hy)
        assert not got[3].any()                   # no counted row and no decay: the gradient is exactly 0


# ---- 3. the gradient is the right gradient ------------------------------------------------------------------------------------------------
def gradient_distances(lib, B, H):
    """(d32, the rule's distance): max |g - g64| / max |g64| of torch's float32 autograd and of gbl_cpu_train_step's grad_out."""
    obs, mask, visits, z = R.random_batch(B, 11 * B + H)
    p, m, v = fresh(H)
    hy = R.hyper_at(1)
    g64, lp64, lv64 = R.torch_gradient(obs, mask, visits, z, H, p, float(hy["weight_decay"]), float(hy["value_reg"]), torch.float64)
    g32, _, _ = R.torch_gradient(obs, mask, visits, z, H, p, float(hy["weight_decay"]), float(hy["value_reg"]), torch.float32)
    got = R.run_step(lib, obs, mask, visits, z, H, p, m, v, hy)
    scale = np.abs(g64).max()
    assert abs(got[4][0] - lp64) <= 1e-5 * max(1.0, lp64) and abs(got[4][1] - lv64) <= 1e-5 * max(1.0, lv64)
    return float(np.abs(g32.astype(np.float64) - g64).max() / scale), float(np.abs(got[3].astype(np.float64) - g64).max() / scale)


@pytest.mark.parametrize("B,H", SHAPES)
def test_gradient_against_float64_autograd(cpu, B, H):
    """The rule gets 8 x d32: three bits for its other summation order and its polynomial exp, each a few ulp per operation.
    Measured (d32, the rule) per shape: profiles/r17/train_step.json."""
    d32, mine = gradient_distances(cpu, B, H)
    print("B %d H %d: torch float32 %.3e, gbl_cpu_train_step %.3e of max |g64|" % (B, H, d32, mine))
    assert d32 > 0 and mine <= 8 * d32


# ---- 4. Adam -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 256])
def test_adam_against_the_float64_formula(cpu, H):
    """From the rule's own grad_out the float64 formula (on the float32 hyper-parameters) gives params, m and v to 4 ulp: each is at
    most four correctly rounded operations deep.  An ulp is that of the larger operand of the element's last add or subtract, which
    is where a float32 result's error lives when the two nearly cancel."""
    obs, mask, visits, z = R.random_batch(65, 9)
    p, m, v = fresh(H)
    for t in (1, 2, 3):
        hy = R.hyper_at(t)
        p2, m2, v2, g, _ = R.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy)
        h = {k: float(x) for k, x in hy.items()}
        g64, p64, a, b = g.astype(np.float64), p.astype(np.float64), h["beta1"] * m.astype(np.float64), 0.0
        b = (1.0 - h["beta1"]) * g64
        m64 = a + b
        v64 = h["beta2"] * v.astype(np.float64) + (1.0 - h["beta2"]) * g64 * g64
        step = h["lr"] * (m64 / h["bias1"]) / (np.sqrt(v64 / h["bias2"]) + h["eps"])
        for name, got, ref, size in (("m", m2, m64, np.maximum(np.abs(a), np.abs(b))), ("v", v2, v64, v64),
                                     ("params", p2, p64 - step, np.maximum(np.abs(p64), np.abs(step)))):
            ulp = np.spacing(np.maximum(size, 2.0 ** -126).astype(F)).astype(np.float64)
            worst = (np.abs(got.astype(np.float64) - ref) / ulp).max()
            print("H %d step %d %s: %.2f ulp" % (H, t, name, worst))
            assert worst <= 4.0, (name, t)
        p, m, v = p2, m2, v2


# ---- 5. exp and log -------------------------------------------------------------------------------------------------------------------------
def ulps(got, ref64):
    """|got - ref| in units of the float32 spacing at ref (the denormal spacing below the normals)."""
    spacing = np.maximum(np.spacing(np.abs(ref64.astype(F))).astype(np.float64), 2.0 ** -149)
    return np.abs(got.astype(np.float64) - ref64) / spacing


@pytest.fixture(scope="module")
def library_math(tmp_path_factory):
    """The library's own train_exp / train_log (gobblet_device.h), compiled for the host with the host flavour's compiler and flags
    behind two array-in / array-out wrappers (tests/emu/train_math.cpp)."""
    import ctypes as C
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    so = str(tmp_path_factory.mktemp("train_math") / "libtrain_math.so")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.check_call([cxx, *nat.CPU_CXX_FLAGS, "-o", so, os.path.join(here, "emu", "train_math.cpp")])
    L = C.CDLL(so)

    def run(name, x):
        x = np.ascontiguousarray(x, F)
        out = np.empty_like(x)
        getattr(L, name)(C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), C.c_int64(x.size))
        return out
    return run


def test_exp_and_log_error_in_ulp(library_math):
    """The error of a fixed polynomial is a fact: 2^20 evenly spaced arguments and the range edges, run through the LIBRARY's functions
    (equal to the restatement's bit for bit on every argument).  The maxima, asserted as the bound and stated in the header and in
    DESIGN 5.16: exp 0.99491 ulp at x = -16.974144 on [-104, 0] (down to where the result leaves the denormals), log 0.74746 ulp at
    s = 1.414164 on [1, 54]."""
    x = np.concatenate([np.linspace(-104.0, 0.0, 1 << 20), [-104.0, 0.0, -103.97, -87.33654, -87.34]]).astype(F)
    s = np.concatenate([np.linspace(1.0, 54.0, 1 << 20), [1.0, 54.0, np.sqrt(2.0), 2.0, 4.0]]).astype(F)
    ex, lg = library_math("train_math_exp", x), library_math("train_math_log", s)
    assert np.array_equal(ex.view(np.uint32), R.exp32(x).view(np.uint32)) and np.array_equal(lg.view(np.uint32), R.log32(s).view(np.uint32))
    e, l = ulps(ex, np.exp(x.astype(np.float64))), ulps(lg, np.log(s.astype(np.float64)))
    print("exp: %.6f ulp at %r; log: %.6f ulp at %r" % (e.max(), x[e.argmax()], l.max(), s[l.argmax()]))
    assert e.max() <= 0.99491 and l.max() <= 0.74746
    assert x[e.argmax()] == F(-16.974144) and s[l.argmax()] == F(1.414164)
    assert library_math("train_math_exp", [0.0, -0.0]).tolist() == [1.0, 1.0] and library_math("train_math_log", [1.0])[0] == 0.0
    assert library_math("train_math_exp", [-104.0, -200.0, -np.inf, np.nan]).tolist() == [0.0, 0.0, 0.0, 0.0]
    assert R.exp32(np.array([-104.0, -200.0, -np.inf], F)).tolist() == [0.0, 0.0, 0.0]


def test_the_library_runs_the_restated_exp_and_log(cpu):
    """One candidate pair per row makes p_1 = EXP(-d) / (1 + EXP(-d)) visible in do: the library's exp, bit for bit, over a sweep."""
    d = np.linspace(0.0, 104.0, 64).astype(F)
    B = len(d)
    obs, mask, visits, z = np.zeros((B, 117), np.int8), np.zeros((B, 54), np.int8), np.zeros((B, 54), np.int16), np.ones(B, np.int8)
    mask[:, :2], visits[:, 0] = 1, 1
    obs[np.arange(B), np.arange(B)] = 1             # row r sets byte r alone: o_1 = -w1[r][0] * 1 below
    p, m, v = (np.zeros(R.param_count(64), F) for _ in range(3))
    w1, b1, w2, b2 = R.split(p, 64)
    w1[:B, 0], w2[0, 1] = d, -1.0
    hy = R.hyper_at(1)
    got = R.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy)
    R.same_bits(got, R.restate_step(obs, mask, visits, z, 64, p, m, v, hy))
    rows = R.restate_rows(obs, mask, visits, z, 64, p, hy["value_reg"])
    e = R.exp32(-d)
    assert np.array_equal(rows["do"][:, 1], e / (F(1) + e)) and (e[-3:] < 2.0 ** -126).all() and e[-1] == 0


# ---- 6. it learns ----------------------------------------------------------------------------------------------------------------------------
def test_a_fit_learns_and_its_evaluator_builds(open_positions):  # noqa: F811
    boards, plies = 128, 17                        # 2 048 plies with a target slot
    env = G.BatchedGobblet(boards, "cpu", auto_reset=True, seed=5, track_turn=True)
    traj = env.collect(plies, policies=("tree", "tree"), search=dict(iterations=16, playouts=2, sample_plies=4))
    env.outcome_targets(traj)
    trainer = G.GobbletTrainer(hidden=64, device="cpu", seed=0)
    stats = env.fit(traj, trainer, 200).numpy()
    assert stats.shape == (200, 4) and np.isfinite(stats).all() and (stats[:, 2] > 900).all() and trainer.t == 200
    loss = stats[:, 0] + stats[:, 1]
    print("loss %.4f at step 0, %.4f at step 199; hidden max %.3f" % (loss[0], loss[-1], float(trainer.hidden_max)))
    assert loss[-10:].mean() < loss[0] and float(trainer.hidden_max) == stats[:, 3].max()
    ev = trainer.evaluator()                        # (raises if a shift leaves 0 .. 24)
    assert all(0 <= s <= 24 for s in (ev.shift1, ev.shift_p, ev.shift_v))
    st, tm = open_positions
    weights = tuple(np.asarray(w, np.float64) for w in trainer.weights())
    compare_with_float(ev, weights, st, tm, rounding=True)
    # the state round-trips, and a reloaded trainer steps to the same bits
    other = G.GobbletTrainer(hidden=64, device="cpu", seed=1)
    other.load_state_dict(trainer.state_dict())
    a = env.fit(traj, trainer, 2, first_call=200)
    b = env.fit(traj, other, 2, first_call=200)
    assert torch.equal(a, b) and torch.equal(trainer.params, other.params) and torch.equal(trainer.last_grad, other.last_grad)


def test_the_trainer_starts_as_torch_linear_does():
    t = G.GobbletTrainer(hidden=128, device="cpu", seed=3)
    state = torch.random.get_rng_state()
    torch.manual_seed(3)
    l1, l2 = torch.nn.Linear(117, 128), torch.nn.Linear(128, 55)
    torch.random.set_rng_state(state)
    w1, b1, w2, b2 = t.weights()
    assert torch.equal(w1, l1.weight.detach().T) and torch.equal(b1, l1.bias.detach())
    assert torch.equal(w2, l2.weight.detach().T) and torch.equal(b2, l2.bias.detach())
    assert t.params.numel() == R.param_count(128) and t.params.data_ptr() % 16 == 0
    with pytest.raises(ValueError):
        G.GobbletTrainer(hidden=100, device="cpu")


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_replay_the_recorded_table(golden_dir):
    """tests/golden/train_arg_errors.json as the other *_arg_errors.json tables: every call returns before any work (the pointers are
    numbers, never read); a case whose "host" is null is an alignment rule, which only the device flavour has."""
    table = json.load(open(os.path.join(golden_dir, "train_arg_errors.json")))
    assert len(table) > 25 and {c["fn"] for c in table} == {"train_step"}
    assert {c["device"][0] for c in table} == {nat.ERR_ARG, nat.ERR_ALIGN}
    assert all(c[f] is None or c[f][0] != nat.OK for c in table for f in ("device", "host"))  # (so the message is compared for every case)
    replay_arg_errors(table)


def test_workspace_bytes_is_positive_and_monotone():
    size = nat.lib().gbl_train_workspace_bytes
    hs, bs = (64, 128, 192, 256), (1, 2, 63, 64, 65, 1024, 65535, 65536)
    for h in hs:
        for b in bs:
            assert size(b, h) == 4 * b * (2 * h + 60) > 0   # (the header's formula)
    assert all(size(b, h0) < size(b, h1) for b in bs for h0, h1 in zip(hs, hs[1:]))
    assert all(size(b0, h) < size(b1, h) for h in hs for b0, b1 in zip(bs, bs[1:]))
    assert [size(0, 64), size(65537, 64), size(8, 100), size(-1, 64)] == [0, 0, 0, 0]
