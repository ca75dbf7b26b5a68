"""gbl_train_step_weighted and gbl_replay_importance, host flavour (no GPU): against gbl_cpu_train_step with weights of 1, against the
numpy-float32 restatement of the header's additions (tests/train_weighted_restatement.py) bit for bit, a weight of 0 against an open
row, the gradient against float64 autograd of the weighted loss, the two per-row outputs, the importance weights with their LOG and
float64 bounds, the Python surface (GobbletTrainer.step(weights=, priority=), ReplayBuffer.batch_weights, fit(beta=, priority=))
and the argument errors."""
import json
import os

import numpy as np
import pytest
import torch

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests import train_restatement as R
from tests import train_weighted_restatement as W
from tests.search_harness import replay_arg_errors

F = np.float32
SHAPES = [(b, h) for b in (1, 3, 65, 130) for h in (64, 256)]
PRIO = (1000.0, 1, 100000)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r26", "train_weighted.json")


@pytest.fixture(scope="module")
def cpu():
    L = nat.cpu_raw()
    L.gbl_cpu_set_threads(4)
    yield L
    L.gbl_cpu_set_threads(0)


def fresh(hidden):
    p = R.init_params(hidden, hidden)
    return p, np.zeros_like(p), np.zeros_like(p)


# ---- 1. weights of 1 are gbl_cpu_train_step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", SHAPES)
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("steps", [1, 20])
def test_weights_null_and_weights_of_one_equal_the_unweighted_step(cpu, B, H, with_mask, steps):
    p, m, v = fresh(H)
    for t in range(1, steps + 1):
        obs, mask, visits, z = R.random_batch(B, 7 * B + H + t, with_mask)
        hy = R.hyper_at(t)
        plain = R.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy)
        W.same_bits(W.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, None, PRIO), plain, (B, H, t, "NULL"))
        W.same_bits(W.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, np.ones(B, F), None, row_loss=False), plain, (B, H, t, "ones"))
        p, m, v = plain[:3]


# ---- 2. bits against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", SHAPES)
@pytest.mark.parametrize("with_mask", [True, False])
@pytest.mark.parametrize("steps", [1, 20])
def test_bits_equal_the_restatement(cpu, B, H, with_mask, steps):
    """Random weights in (0, 4] with a 0, a denormal, -1, NaN and +inf among them (from 8 rows on), every output."""
    p, m, v = fresh(H)
    for t in range(1, steps + 1):
        obs, mask, visits, z = R.random_batch(B, 5 * B + H + t, with_mask)
        w, hy = W.random_weights(B, B + t), R.hyper_at(t)
        got = W.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, w, PRIO)
        W.same_bits(got, W.restate_step(obs, mask, visits, z, H, p, m, v, hy, w, PRIO), (B, H, with_mask, t))
        assert got[4][2] == (B if B < 4 else B - 2) and np.isfinite(got[4]).all()   # (a weight of 0 still counts in N)
        p, m, v = got[:3]


def test_minus_one_nan_and_inf_behave_as_zero(cpu):
    obs, mask, visits, z = R.random_batch(65, 21)
    p, m, v = fresh(64)
    hy = R.hyper_at(1)
    w = W.random_weights(65, 3)
    assert w[0] == 0 and 0 < w[3] < 2.0 ** -126 and w[4] == -1 and np.isnan(w[5]) and np.isinf(w[7])
    assert W.effective(w, 65)[[0, 4, 5, 7]].tolist() == [0, 0, 0, 0] and W.effective(w, 65)[3] == w[3]
    zeroed = w.copy()
    zeroed[[4, 5, 7]] = 0
    W.same_bits(W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, w, PRIO), W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, zeroed, PRIO))
    assert all(np.isfinite(a).all() for a in W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, w, PRIO)[:6])


@pytest.mark.parametrize("edge", ["none counted", "open rows", "one candidate"])
def test_edge_batches_equal_the_restatement(cpu, edge):
    obs, mask, visits, z, H, p, _ = R.EDGES[edge]()
    m, v, hy = np.zeros_like(p), np.zeros_like(p), R.hyper_at(1)
    w = W.random_weights(len(obs), 11, special=False)
    got = W.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, w, PRIO)
    W.same_bits(got, W.restate_step(obs, mask, visits, z, H, p, m, v, hy, w, PRIO), edge)
    if edge == "none counted":
        assert not got[5].any() and not got[6].any() and np.array_equal(got[4], np.zeros(4, F))


# ---- 3. a weight of 0 against an open row -----------------------------------------------------------------------------------------------
def test_weight_zero_against_an_open_row_is_exact(cpu):
    """The same G sums over 128 counted rows (M = 128) and over 64 (M = 64): 2 g_weighted == g_open bit for bit wherever g is far from
    the denormals."""
    B = 128
    obs, mask, visits, z = R.random_batch(B, 33)
    z[1], visits[2] = 1, visits[4]                       # (every row counts)
    p, m, v = fresh(64)
    hy = R.hyper_at(1, weight_decay=0.0)
    w = np.ones(B, F)
    w[1::2] = 0
    got = W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, w)
    z_open = z.copy()
    z_open[1::2] = R.Z_OPEN
    ref = R.run_step(cpu, obs, mask, visits, z_open, 64, p, m, v, hy)
    assert got[4][2] == 128 and ref[4][2] == 64
    big = np.abs(ref[3]) >= 2.0 ** -100
    assert big.sum() > 1000 and np.array_equal((F(2) * got[3])[big].view(np.uint32), ref[3][big].view(np.uint32))


# ---- 4. the gradient is the weighted loss's gradient ---------------------------------------------------------------------------------------
def record(key, value):
    """One entry of profiles/r26/train_weighted.json, where the file is writable (a measurement; nothing reads it back)."""
    try:
        data = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
        data.setdefault("host_tests", {})[key] = value
        with open(PROFILE, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


@pytest.mark.parametrize("B,H", SHAPES)
def test_gradient_against_float64_autograd(cpu, B, H):
    """max |g - g64| / max |g64| of the rule is within 8 x that of torch's own float32 autograd on the same inputs (5.16's rule).
    Measured per shape: profiles/r26/train_weighted.json."""
    obs, mask, visits, z = R.random_batch(B, 13 * B + H)
    w = W.random_weights(B, B + H)
    p, m, v = fresh(H)
    hy = R.hyper_at(1)
    wd, vr = float(hy["weight_decay"]), float(hy["value_reg"])
    g64 = W.torch_gradient(obs, mask, visits, z, H, p, w, wd, vr, torch.float64)
    g32 = W.torch_gradient(obs, mask, visits, z, H, p, w, wd, vr, torch.float32)
    got = W.run_step(cpu, obs, mask, visits, z, H, p, m, v, hy, w)
    scale = np.abs(g64).max()
    d32, mine = float(np.abs(g32.astype(np.float64) - g64).max() / scale), float(np.abs(got[3].astype(np.float64) - g64).max() / scale)
    print("B %d H %d: torch float32 %.3e, gbl_cpu_train_step_weighted %.3e of max |g64|" % (B, H, d32, mine))
    record("gradient B=%d H=%d" % (B, H), {"torch_float32": d32, "gbl_cpu_train_step_weighted": mine})
    assert d32 > 0 and mine <= 8 * d32


# ---- 5. prio_out and row_loss_out -----------------------------------------------------------------------------------------------------------
def test_row_loss_out_sums_to_the_statistics(cpu):
    obs, mask, visits, z = R.random_batch(130, 41)
    p, m, v = fresh(64)
    got = W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, R.hyper_at(1), np.ones(130, F))
    total = np.zeros(2, F)
    for r0 in range(0, 130, R.CHUNK):
        acc = np.zeros(2, F)
        for r in range(r0, min(130, r0 + R.CHUNK)):
            acc = acc + got[5][r]
        total = total + acc
    M = got[4][2]
    assert M == 128 and np.array_equal((total / M).view(np.uint32), got[4][:2].view(np.uint32))
    assert not got[5][[1, 2]].any() and (got[5][[0, 3]] > 0).all()


@pytest.mark.parametrize("prio", [(0.0, 3, 9), (1e30, 2, 77), (1000.0, 5, 5), (1000.0, 0, 2 ** 31 - 1), (3e9, 2 ** 31 - 1, 2 ** 31 - 1),
                                  (1e-30, 1, 10)], ids=str)
def test_prio_out_equals_the_restatement(cpu, prio):
    obs, mask, visits, z = R.random_batch(65, 43)
    p, m, v = fresh(64)
    hy = R.hyper_at(1)
    got = W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, None, prio)
    exp = W.restate_step(obs, mask, visits, z, 64, p, m, v, hy, None, prio)
    W.same_bits(got, exp, prio)
    counted = np.ones(65, bool)
    counted[[1, 2]] = False
    assert not got[6][~counted].any()
    scale, floor, cap = prio
    if scale == 0.0 or scale == 1e-30:
        assert (got[6][counted] == floor).all()          # every counted row at the floor
    if scale in (1e30, 3e9) or floor == cap:
        assert (got[6][counted] == cap).all()            # past 2^30 (or floor = cap): every counted row at the cap
    if prio == (1000.0, 0, 2 ** 31 - 1):
        lo = got[5][counted].sum(1)
        assert np.array_equal(got[6][counted], ((got[5][counted, 0] + got[5][counted, 1]) * F(1000)).astype(np.int32)) and lo.min() > 0


def test_the_two_outputs_do_not_depend_on_the_weights(cpu):
    obs, mask, visits, z = R.random_batch(65, 47)
    p, m, v = fresh(64)
    hy = R.hyper_at(1)
    a = W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, W.random_weights(65, 1), PRIO)
    b = W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, W.random_weights(65, 2, special=False), PRIO)
    c = W.run_step(cpu, obs, mask, visits, z, 64, p, m, v, hy, None, PRIO)
    assert a[5].tobytes() == b[5].tobytes() == c[5].tobytes() and a[6].tobytes() == b[6].tobytes() == c[6].tobytes()
    assert a[3].tobytes() != b[3].tobytes()


# ---- 6. gbl_cpu_replay_importance ------------------------------------------------------------------------------------------------------------
def priorities(n, seed):
    """Log-uniform int32 priorities with duplicates, zeros and negatives mixed in."""
    rng = np.random.default_rng(seed)
    p = np.exp(rng.uniform(0.0, np.log(2.0 ** 31 - 1), n)).astype(np.int64).clip(1, 2 ** 31 - 1).astype(np.int32)
    if n >= 8:
        p[1], p[2], p[5], p[6] = p[0], 0, -3, np.iinfo(np.int32).min
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_importance_equals_the_restatement(cpu, n):
    for seed, beta in enumerate((0.0, 0.25, 0.4, 0.5, 1.0)):
        p = priorities(n, 100 * n + seed)
        got = W.run_importance(cpu, p, beta)
        assert np.array_equal(got.view(np.uint32), W.restate_importance(p, beta).view(np.uint32)), (n, beta)
        pos = p > 0
        assert not got[~pos].any() and (got[p == p[pos].min()] == 1.0).all() and (got[pos] > 0).all() and (got <= 1.0).all()
        if beta == 0.0:
            assert (got[pos] == 1.0).all()
        if n >= 8:
            assert got[0] == got[1]                         # (duplicate priorities)
        dead = -np.abs(p)
        dead[::3] = 0
        assert not W.run_importance(cpu, dead, beta).any()   # no entry positive: every weight 0


@pytest.fixture(scope="module")
def library_math(tmp_path_factory):
    """The library's own scalar pieces (gobblet_device.h) compiled for the host with the host flavour's compiler and flags
    (tests/emu/train_weighted_math.cpp)."""
    import ctypes as C
    import shutil
    import subprocess
    so = str(tmp_path_factory.mktemp("train_weighted_math") / "libtrain_weighted_math.so")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.check_call([cxx, *nat.CPU_CXX_FLAGS, "-o", so, os.path.join(ROOT, "tests", "emu", "train_weighted_math.cpp")])
    return C.CDLL(so)


def test_log_error_in_ulp_up_to_2_31(library_math):
    """The error of train_log on [1, 2^31], where gbl_replay_importance uses it: 2^20 evenly spaced arguments and the range edges
    through the LIBRARY's function (equal to the restatement's bit for bit) -- 0.60622 ulp at s = 1.4142135 -- and, because so wide a
    grid hardly samples the first octaves, the 2^20 arguments of [1, 54] that tests/test_train_step.py measures as well.  The maximum
    of both, asserted as the bound and stated in the header and in DESIGN 5.24: 0.74746 ulp at s = 1.414164."""
    import ctypes as C
    from tests.test_train_step import ulps
    wide = np.concatenate([np.linspace(1.0, 2.0 ** 31, 1 << 20), [1.0, 2.0 ** 31, 2.0, np.sqrt(2.0), 2.0 ** 30, 2.0 ** 31 - 128]]).astype(F)
    s = np.concatenate([wide, np.linspace(1.0, 54.0, 1 << 20).astype(F)])
    out = np.empty_like(s)
    library_math.train_math_log(C.c_void_p(s.ctypes.data), C.c_void_p(out.ctypes.data), C.c_int64(s.size))
    assert np.array_equal(out.view(np.uint32), R.log32(s).view(np.uint32))
    err = ulps(out, np.log(s.astype(np.float64)))
    far = err[:wide.size]
    print("log on [1, 2^31]: %.6f ulp at %r on the wide grid, %.6f ulp at %r with [1, 54]'s" % (far.max(), wide[far.argmax()], err.max(), s[err.argmax()]))
    record("log_ulp_1_to_2_31", {"wide_grid_max_ulp": float(far.max()), "wide_grid_at": float(wide[far.argmax()]),
                                 "max_ulp": float(err.max()), "at": float(s[err.argmax()])})
    assert far.max() <= 0.60622 and err.max() <= 0.74746 and s[err.argmax()] == F(1.414164)
    # the scalar pieces of the rule, the library's against the restatement's
    w = np.array([0.0, -0.0, 1e-41, -1.0, np.nan, np.inf, -np.inf, 3.5, np.finfo(F).max, 1.0], F)
    got = np.empty_like(w)
    library_math.train_math_weight(C.c_void_p(w.ctypes.data), C.c_void_p(got.ctypes.data), C.c_int64(w.size))
    assert np.array_equal(got.view(np.uint32), W.effective(w, len(w)).view(np.uint32))


def test_importance_against_float64(cpu):
    """Against float64 (wmin / w)^beta and against ReplayBuffer.importance_weights over the test's inputs.  The bound is the measured
    maximum relative error (1.035e-6 of float64 and 1.075e-6 of importance_weights, both at beta = 1: a LOG of up to 21.5 within an
    ulp of 1.9e-6, through an EXP within an ulp) rounded up to the next power of two, 2^-19."""
    worst = {}
    for seed, beta in enumerate((0.25, 0.4, 0.5, 1.0)):
        p = priorities(1 << 16, 7 + seed)
        got = W.run_importance(cpu, p, beta).astype(np.float64)
        pos = p > 0
        ref = np.where(pos, (p[pos].min() / np.where(pos, p, 1).astype(np.float64)) ** float(F(beta)), 0.0)
        batch = {"priority": torch.from_numpy(p), "prio_total": torch.tensor([int(p[pos].astype(np.int64).sum()), 1 << 20], dtype=torch.int64)}
        tw = G.ReplayBuffer.importance_weights(batch, float(F(beta))).numpy().astype(np.float64)
        rel, rel_t = np.abs(got - ref)[pos] / ref[pos], np.abs(got - tw)[pos] / ref[pos]
        assert not got[~pos].any() and not tw[~pos].any()
        worst[str(beta)] = {"float64": float(rel.max()), "importance_weights": float(rel_t.max())}
        print("beta %g: %.3e of float64, %.3e of importance_weights" % (beta, rel.max(), rel_t.max()))
        assert rel.max() <= 2.0 ** -19 and rel_t.max() <= 2.0 ** -19
    record("importance_relative_error", worst)


# ---- 7. the Python surface ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ring():
    env = G.BatchedGobblet(64, "cpu", auto_reset=True, seed=5, track_turn=True)
    traj = env.collect(8, policies=("tree", "tree"), search=dict(iterations=8, playouts=2, sample_plies=4))
    env.outcome_targets(traj)

    def make():
        buf = G.ReplayBuffer(1024, "cpu", prioritized=True)
        buf.append(env, traj, tag=1, priority=7)
        return buf
    return make


PRIORITY = dict(scale=1000, floor=1, cap=100000)


def test_fit_with_beta_and_priority_equals_the_hand_written_loop(ring):
    a, b = ring(), ring()
    ta, tb = G.GobbletTrainer(hidden=64, device="cpu", seed=1), G.GobbletTrainer(hidden=64, device="cpu", seed=1)
    before = a.priority.clone()
    stats = a.fit(ta, 8, batch=64, first_call=3, prioritized=True, beta=0.5, priority=PRIORITY)
    by_hand, drawn = [], set()
    for i in range(8):
        buf = b.batch(64, call=3 + i, prioritized=True)
        w = b.batch_weights(buf, 0.5)
        by_hand.append(tb.step(buf, weights=w, priority=PRIORITY))
        b.set_priority(buf["index"], tb.last_priority)
        drawn |= set(buf["index"][:, 0].tolist())
    assert torch.equal(stats, torch.stack(by_hand)) and stats.shape == (8, 4) and float(stats[:, 2].min()) == 64
    for x, y in ((ta.params, tb.params), (ta.m, tb.m), (ta.v, tb.v), (a.priority, b.priority)):
        assert x.numpy().tobytes() == y.numpy().tobytes()
    size = a.size
    never = torch.tensor([s for s in range(size) if s not in drawn])
    assert 0 < len(never) < size and torch.equal(a.priority[never], before[never]) and (before[:size] == 7).all()
    touched = torch.tensor(sorted(drawn))
    assert (a.priority[touched] >= 1).all() and (a.priority[touched] != 7).any() and not a.priority[size:].any()
    assert ta.last_row_loss.shape == (64, 2) and ta.last_row_loss.dtype == torch.float32 and ta.last_priority.dtype == torch.int32
    loss = ta.last_row_loss.sum(1)
    assert torch.equal(ta.last_priority, torch.clamp(1 + (loss * 1000).to(torch.int32), max=100000))


def test_an_annealed_beta_and_each_argument_alone(ring):
    a, b = ring(), ring()
    ta, tb = G.GobbletTrainer(hidden=64, device="cpu", seed=2), G.GobbletTrainer(hidden=64, device="cpu", seed=2)
    a.fit(ta, 3, batch=32, prioritized=True, beta=(0.4, 1.0))
    for i, beta in enumerate((0.4, 0.7, 1.0)):
        buf = b.batch(32, call=i, prioritized=True)
        tb.step(buf, weights=b.batch_weights(buf, 0.4 + (1.0 - 0.4) * (i / 2)))
    assert torch.equal(ta.params, tb.params) and torch.equal(a.priority, b.priority) and ta.last_priority is None
    a.fit(ta, 2, batch=32, first_call=3, prioritized=True, priority=PRIORITY)      # priority alone: unweighted steps, priorities move
    for i in range(2):
        buf = b.batch(32, call=3 + i, prioritized=True)
        tb.step(buf, priority=PRIORITY)
        b.set_priority(buf["index"], tb.last_priority)
    assert torch.equal(ta.params, tb.params) and torch.equal(a.priority, b.priority) and not torch.equal(a.priority, ring().priority)
    buf = a.batch(32, call=9, prioritized=True)
    w = a.batch_weights(buf, 0.5)
    assert a.batch_weights(buf, 0.5, out=w) is w and w.dtype == torch.float32 and w.shape == (32,)
    assert torch.allclose(w, G.ReplayBuffer.importance_weights(buf, 0.5), rtol=2.0 ** -19, atol=0)


def test_beta_and_priority_need_prioritized_and_their_arguments_are_checked(ring):
    buf, t = ring(), G.GobbletTrainer(hidden=64, device="cpu", seed=1)
    for kw in (dict(beta=0.5), dict(priority=PRIORITY), dict(beta=0.5, priority=PRIORITY)):
        with pytest.raises(ValueError, match="prioritized=True"):
            buf.fit(t, 1, batch=16, **kw)
    drawn = buf.batch(16, prioritized=True)
    for bad in (dict(weights=torch.ones(15)), dict(weights=torch.ones(16, dtype=torch.float64)), dict(priority=dict(scale=1.0)),
                dict(priority=dict(scale=-1.0, cap=5)), dict(priority=dict(scale=1.0, floor=6, cap=5)),
                dict(priority=dict(scale=1.0, cap=5, alpha=0.6))):
        with pytest.raises(ValueError):
            t.step(drawn, **bad)
    with pytest.raises(ValueError):
        buf.batch_weights(drawn, 1.5)
    with pytest.raises(ValueError):
        buf.batch_weights(buf.batch(16), 0.5)
    with pytest.raises(ValueError):
        G.ReplayBuffer(64, "cpu").batch_weights(drawn, 0.5)
    assert t.t == 0


def test_fit_without_the_new_arguments_is_what_it_was(ring):
    a, b = ring(), ring()
    ta, tb = G.GobbletTrainer(hidden=64, device="cpu", seed=1), G.GobbletTrainer(hidden=64, device="cpu", seed=1)
    stats = a.fit(ta, 4, batch=64, first_call=2, prioritized=True)
    by_hand = torch.stack([tb.step(b.batch(64, call=2 + i, prioritized=True)) for i in range(4)])
    assert torch.equal(stats, by_hand) and torch.equal(ta.params, tb.params) and ta.last_row_loss is None and ta.last_priority is None
    stats = a.fit(ta, 2, batch=64, first_call=9)
    by_hand = torch.stack([tb.step(b.batch(64, call=9 + i)) for i in range(2)])
    assert torch.equal(stats, by_hand) and torch.equal(ta.params, tb.params) and torch.equal(a.priority, b.priority)


def test_the_per_fit_example_runs_on_the_host_flavour():
    import importlib.util
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    spec = importlib.util.spec_from_file_location("example_per_fit", os.path.join(ROOT, "examples", "example_per_fit.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    log = ex.per_fit("cpu", inventory=(2, 2, 0), windows=2, boards=128, plies=12, steps=3, batch=128, iterations=8, capacity=2048, held_out=256)
    assert set(log) == {"rows", "uniform", "regret_table", "loss_driven"} and log["rows"] > 0
    assert log["uniform"]["rows"] == log["regret_table"]["rows"] == log["loss_driven"]["rows"] > 0
    assert all(0.0 <= log[k][s] <= 1.0 for k in ex.FITS for s in ("value_sign", "top_prior_in_R"))


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_replay_the_recorded_table(golden_dir):
    """tests/golden/train_weighted_arg_errors.json (scripts/record_train_weighted_arg_errors.py): every call returns before any work
    (the pointers are numbers, never read); a case whose "host" is null is an alignment rule, which only the device flavour has."""
    table = json.load(open(os.path.join(golden_dir, "train_weighted_arg_errors.json")))
    assert len(table) > 40 and {c["fn"] for c in table} == {"train_step_weighted", "replay_importance"}
    assert {c["device"][0] for c in table} == {nat.ERR_ARG, nat.ERR_ALIGN}
    assert all(c[f] is None or c[f][0] != nat.OK for c in table for f in ("device", "host"))
    replay_arg_errors(table)
    # prio_scale, prio_floor and prio_cap are read only when prio_out is given: the same bad values without it are a good call
    obs, mask, visits, z = R.random_batch(3, 1)
    p, m, v = fresh(64)
    L = nat.cpu_raw()
    assert W.run_step(L, obs, mask, visits, z, 64, p, m, v, R.hyper_at(1), None, None, unread=(-1.0, 5, 4))[4][2] == 3
