"""CPU-side checks of the product's host code: the C-ABI library builds, loads and exports every
symbol include/gobblet_hip.h declares (no compute call is made without a GPU); argument checks
that do not need a device; the single-env AEC facade's turn logic against the golden trajectories
(the CPU tests monkeypatch the facade's private engine factory with a test-only oracle board)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import gobblet_rl_amd as G
from gobblet_rl_amd import _native as nat
from tests.oracle_backend import OracleBoardEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_all_exported():
    hdr = open(os.path.join(ROOT, "include", "gobblet_hip.h")).read()
    declared = set(re.findall(r"\b(gbl_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(nat.SIGNATURES), (declared ^ set(nat.SIGNATURES))
    L = nat.lib()  # builds with hipcc if needed, loads, resolves every symbol
    for name in declared:
        assert getattr(L, name) is not None


def test_selfplay_args_are_the_headers_declarations():
    """nat.SELFPLAY_ARGS -- the one place the Python side takes the self-play family's argument order from -- against the seven
    declarations of include/gobblet_hip.h, parameter by parameter: the name, and the ctype of its C type.  (gobblet_cpu.h is held
    against gobblet_hip.h textually below, so all fourteen declarations are pinned.)"""
    hdr = open(os.path.join(ROOT, "include", "gobblet_hip.h")).read()
    ctype_of = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}
    family = set(re.findall(r"^int (gbl_collect_search[a-z_]*)\(", hdr, re.M))
    assert family == set(nat.SELFPLAY_ARGS) and len(family) == 7, family ^ set(nat.SELFPLAY_ARGS)
    for name, table in nat.SELFPLAY_ARGS.items():
        declared = []
        for param in re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M).group(1).split(","):
            ctype, pointer, param_name = re.fullmatch(r"\s*(?:const )?(\w+) (\*?)(\w+)\s*", param).groups()
            declared.append((param_name, C.c_void_p if pointer else ctype_of[ctype]))
        assert declared == list(table), (name, [(d, t) for d, t in zip(declared, table) if d != t], len(declared), len(table))
        assert nat.SIGNATURES[name] == (C.c_int, [t for _, t in table])
    with pytest.raises(TypeError, match="'turn'"):
        nat.selfplay_args("gbl_collect_search", **{k: None for k, _ in nat.SELFPLAY_ARGS["gbl_collect_search"] if k != "turn"})
    with pytest.raises(TypeError, match="'ev0'"):
        nat.selfplay_args("gbl_collect_search", **{k: None for k, _ in nat.SELFPLAY_ARGS["gbl_collect_search"]}, ev0=None)


def kernel_metadata(lib_path=None):
    """{kernel symbol: {field: value}} from the AMDGPU metadata note of the gfx950 code object embedded in the library."""
    import shutil
    import subprocess
    import tempfile
    tools = "/opt/rocm/lib/llvm/bin"
    lib_path = lib_path or nat.build()
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib_path, os.path.join(tmp, "lib.so"))
        subprocess.run([os.path.join(tools, "llvm-objdump"), "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        objs = [f for f in os.listdir(tmp) if "gfx950" in f]
        assert len(objs) == 1, objs
        notes = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", objs[0]], cwd=tmp, check=True,
                               capture_output=True, text=True).stdout
    out = {}
    for blk in re.findall(r"- \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", notes, re.S):
        fields = dict(re.findall(r"\.(\w+):\s+(\S+)", blk))
        out[fields["name"]] = fields
    return out


def test_no_kernel_uses_scratch():
    """No instantiation of any kernel may spill: a spilled register is a scratch (HBM-backed) round trip per use inside
    the hot loop.  Round 3's k_collect_policy<1, 4> / <1, 16> spilled 22 VGPRs (96 B of scratch per lane) and nothing noticed."""
    meta = kernel_metadata()
    kernels = {k: v for k, v in meta.items() if re.search(r"\dk_[a-z_0-9]+", k)}
    assert len(kernels) > 80 and any("k_collect_policy" in k for k in kernels) and any("k_greedy" in k for k in kernels)
    bad = {k: (v["private_segment_fixed_size"], v["vgpr_spill_count"], v["sgpr_spill_count"]) for k, v in kernels.items()
           if int(v["private_segment_fixed_size"]) or int(v["vgpr_spill_count"])}
    assert not bad, bad
    assert not [k for k, v in kernels.items() if v.get("uses_dynamic_stack") == "true"]  # (a real call into unknown code: scratch)
    # wave64 everywhere, and every workgroup shape fits a CU (<= 512 VGPRs per SIMD lane-slice, 160 KB of LDS)
    for k, v in kernels.items():
        assert v["wavefront_size"] == "64", k
        waves_per_simd = -(-int(v["max_flat_workgroup_size"]) // 64 // 4)
        assert waves_per_simd * (-(-int(v["vgpr_count"]) // 8) * 8) <= 512, (k, v["vgpr_count"], v["max_flat_workgroup_size"])
        assert int(v["group_segment_fixed_size"]) <= 160 * 1024, k


def test_evaluator_selfplay_kernels_keep_their_wavefronts():
    """The evaluator self-play family sits at the edge of its register bands: each instantiation keeps at least the wavefronts per
    SIMD (by VGPRs, in allocation units of 8) it had when its text was folded into shared pieces, and exactly its static LDS.  A change
    that gains a wavefront passes; one that loses a wavefront fails."""
    import subprocess
    floors = {  # demangled name: (wavefronts per SIMD at least, static LDS bytes)
        "k_collect_eval<false>": (4, 448), "k_collect_eval<true>": (4, 448),
        "k_collect_solve<false, false>": (4, 1328), "k_collect_solve<false, true>": (4, 1328),
        "k_collect_solve<true, false>": (4, 1328), "k_collect_solve<true, true>": (4, 1328),
        "k_collect_gumbel_solve": (3, 1328),
        "k_collect_tb<false, false>": (8, 192), "k_collect_tb<false, true>": (3, 1328), "k_collect_tb<true, true>": (3, 1328),
        "k_collect_gumbel_tb": (4, 448),
        "k_tree_eval<false, true>": (4, 256), "k_reanalyse<true>": (4, 256),
    }
    meta = kernel_metadata()
    names = sorted(meta)
    demangled = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    seen = {}
    for k, d in zip(names, demangled):
        d = d.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
        if d in floors:
            seen[d] = (512 // (-(-int(meta[k]["vgpr_count"]) // 8) * 8), int(meta[k]["group_segment_fixed_size"]), meta[k]["vgpr_count"])
    assert sorted(seen) == sorted(floors), sorted(set(floors) - set(seen))
    for d, (waves, lds) in floors.items():
        assert seen[d][0] >= waves, (d, "vgpr", seen[d][2], "wavefronts per SIMD", seen[d][0], "floor", waves)
        assert seen[d][1] == lds, (d, "lds", seen[d][1], lds)


def test_layout_info_and_host_side_argument_errors():
    L = nat.lib()
    info = (C.c_int32 * 6)()
    assert L.gbl_layout_info(info) == 0 and list(info) == [2, 27, 54, 117, 64, 16]
    assert L.gbl_layout_info(None) == nat.ERR_ARG and b"NULL" in L.gbl_last_error()
    # n == 0 is a no-op, n < 0 and NULL pointers are argument errors -- all decided before any HIP call
    assert L.gbl_winner(None, None, 0, None) == 0
    assert L.gbl_winner(None, None, -1, None) == nat.ERR_ARG
    assert L.gbl_winner(None, None, 5, None) == nat.ERR_ARG
    assert L.gbl_legal_mask(16, 16, 24, 5, None) == nat.ERR_ALIGN  # mask pointer not 16-byte aligned
    assert L.gbl_step(16, 16, 16, 16, None, None, None, None, None, 5, 7, 0, None) == nat.ERR_ARG  # bad illegal_mode
    assert L.gbl_greedy(16, 16, None, None, 4, 16, None, None, 5, None) == nat.ERR_ARG       # depth is 1, 2 or 3
    assert L.gbl_greedy(16, 16, None, None, 0, 16, None, None, 5, None) == nat.ERR_ARG
    assert L.gbl_observe(16, None, -1, 16, 5, None) == nat.ERR_ARG                           # needs to_move
    with pytest.raises(nat.GobbletHipError):
        nat.check(nat.ERR_ARG, "x")


def test_env_entry_points_recorded_argument_errors():
    """tests/golden/env_arg_errors.json (scripts/record_env_arg_errors.py): for the env, collect and greedy entry points and the four
    helpers without a host flavour, every check alone, every adjacent pair broken together and the n == 0 / plies == 0 early returns,
    with the return code and the last-error text of either flavour as recorded BEFORE the checks were written once in
    csrc/gobblet_device.h.  Every call returns before any work: no GPU needed."""
    from tests.search_harness import replay_arg_errors
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "env_arg_errors.json")))
    covered = {c["fn"] for c in table}
    assert len(table) > 500 and len(covered) == 31 and {"step", "collect_from_ex", "greedy_act_at", "placement_probe"} <= covered
    for fn in covered:  # (every function has a case of each flavour it has; a function with n has both early-return cases)
        mine = [c for c in table if c["fn"] == fn]
        assert any(c["device"][0] for c in mine), fn
        assert ("gbl_" + fn in nat._NO_HOST_FLAVOUR) == all(c["host"] is None for c in mine), fn
    assert sum(c["device"][0] == nat.ERR_ALIGN for c in table) > 150 and sum(c["device"][0] == 0 for c in table) > 60
    replay_arg_errors(table)


def test_the_host_flavour_is_asked_for_never_fallen_back_to():
    """A GPU device without a GPU is an error -- nothing routes it to the host flavour; "cpu" asks for the host flavour of the
    ABI (include/gobblet_cpu.h) by name; any other device has no flavour."""
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(Exception) as e:
            G.BatchedBoard(8, device="cuda:0")
        assert "_HostFlavour" not in str(e.value)
    b = G.BatchedBoard(8, device="cpu")
    assert type(b._lib).__name__ == "_HostFlavour" and b.squares.device.type == "cpu"
    with pytest.raises(G.GobbletHipError):
        nat.lib_for("meta")
    with pytest.raises(G.GobbletHipError):
        nat.lib_for("cpu").gbl_placement_probe   # the device-memory helpers have no host flavour


def test_host_flavour_header_symbols_all_exported():
    """include/gobblet_cpu.h: every gbl_cpu_* it declares is exported by csrc/libgobblet_cpu.so with the device entry point's
    parameter list, and it covers every compute entry point of gobblet_hip.h."""
    hdr = open(os.path.join(ROOT, "include", "gobblet_cpu.h")).read()
    declared = set(re.findall(r"\b(gbl_cpu_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(nat.CPU_SIGNATURES), declared ^ set(nat.CPU_SIGNATURES)
    L = nat.cpu_raw()
    for name in declared:
        assert getattr(L, name) is not None
    dev_hdr = open(os.path.join(ROOT, "include", "gobblet_hip.h")).read()
    for name in declared - {"gbl_cpu_set_threads"}:
        dev = "gbl_" + name[len("gbl_cpu_"):]
        a = re.search(r"^(?:const char \*|int )" + dev + r"\(([^;]*)\);", dev_hdr, re.M).group(1)
        b = re.search(r"^(?:const char \*|int )" + name + r"\(([^;]*)\);", hdr, re.M).group(1)
        assert re.sub(r"\s+", " ", a) == re.sub(r"\s+", " ", b), name
    info = (C.c_int32 * 6)()
    assert L.gbl_cpu_layout_info(info) == 0 and list(info)[:5] == [2, 27, 54, 117, 64]
    assert L.gbl_cpu_winner(None, None, -1, None) == nat.ERR_ARG and L.gbl_cpu_winner(None, None, 0, None) == 0
    assert L.gbl_cpu_step(16, 16, 16, 16, None, None, None, None, None, 5, 7, 0, None) == nat.ERR_ARG and b"illegal_mode" in L.gbl_cpu_last_error()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "gobblet-rl_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(import|from)\s+(oracle|tests)\b", src, re.M), f
                assert "gobblet_oracle" not in src and "libgobblet_emu" not in src, f
                if f.endswith((".cpp", ".h", ".hip")):
                    assert not re.search(r'#include\s*[<"][^>"]*oracle', src), f   # (the host flavour shares the DEVICE header, nothing else)


# ---- the AEC facade's host logic (gobblet.py:123-290), oracle backend -----------------------------------

@pytest.fixture(autouse=True)
def oracle_engine(monkeypatch):
    """No GPU here: the facade's private engine factory is patched to a CPU stand-in for these host-logic
    tests (the product has no such switch; tests/test_gpu_parity.py runs the same checks on the HIP engine)."""
    monkeypatch.setattr(G.gobblet_v1, "_new_backend", lambda device: OracleBoardEngine())


def make_raw():
    return G.gobblet_v1.raw_env()


def test_reset_starting():  # reference tests/test_gobblet_env.py:23-28
    e = make_raw()
    e.reset()
    assert (e.board.squares == np.zeros(27)).all()
    assert e.agent_selection == "player_1" and e.turn == 0 and e.action == -1 and e.infos == {"player_1": {}, "player_2": {}}


def test_upstream_kat_through_raw_env(golden_dir):  # reference tests/test_manual_policy_collector.py
    kat = json.load(open(os.path.join(golden_dir, "kat_collector.json")))
    e = make_raw()
    e.reset()
    assert e.observe("player_1")["action_mask"].tolist() == kat["mask_after"]["output0"]
    for name, a in zip(["output1", "output2", "output3", "output4"], kat["actions"]):
        e.step(a)
        assert e.observe(e.agent_selection)["action_mask"].tolist() == kat["mask_after"][name]
    assert e._legal_moves() == kat["legal_moves_output6"]
    e.step(kat["illegal_action"])
    assert e.board.squares.astype(int).tolist() == kat["board_output8"]
    assert e.agent_selection == "player_2"  # the turn passes on an illegal move (gobblet.py:244-246)


def test_raw_env_replays_golden_games(golden_dir):
    g = np.load(os.path.join(golden_dir, "random_games.npz"))
    e = make_raw()
    idx = np.flatnonzero(g["game"] < 12)
    for i in idx:
        if g["ply"][i] == 0:
            e.reset()
        assert e.agents.index(e.agent_selection) == g["mover"][i]
        e.step(int(g["action"][i]))
        assert np.array_equal(e.board.squares, g["squares_after"][i])
        nxt = e.agent_selection
        other = e.agents[1 - e.agents.index(nxt)]
        o = e.observe(nxt)
        assert o["observation"].dtype == np.int8 and o["observation"].shape == (3, 3, 13)
        assert np.array_equal(o["action_mask"], g["mask_next"][i])
        assert np.array_equal(e.observe(other)["action_mask"], g["mask_offturn"][i])
        assert np.array_equal(e.observe("player_1")["observation"], g["obs_p1"][i])
        assert np.array_equal(e.observe("player_2")["observation"], g["obs_p2"][i])
        assert [e.rewards["player_1"], e.rewards["player_2"]] == g["reward"][i].tolist()
        assert [e._cumulative_rewards["player_1"], e._cumulative_rewards["player_2"]] == g["cum_reward"][i].tolist()
        assert e.terminations["player_1"] == bool(g["done"][i]) == e.terminations["player_2"]
        assert e.observation_space(nxt).contains(o) and e.turn == g["ply"][i] + 1


def test_aec_loop_like_example_basic():
    """The loop of examples/example_basic.py:50-67 over env(): masked-random play to termination."""
    rng = np.random.default_rng(0)
    e = G.gobblet_v1.env()
    with pytest.raises(AttributeError):
        e.step(0)  # OrderEnforcing: step before reset
    for game in range(5):
        e.reset()
        totals = {"player_1": 0, "player_2": 0}
        steps = 0
        for agent in e.agent_iter():
            observation, reward, termination, truncation, info = e.last()
            totals[agent] += reward
            if termination or truncation:
                e.step(None)
            else:
                mask = observation["action_mask"]
                e.step(int(rng.choice(np.arange(len(mask)), p=mask / np.sum(mask))))
                steps += 1
        assert sorted(totals.values()) == [-1, 1] and steps >= 5 and e.agents == []


def test_env_illegal_move_terminates_with_minus_one():
    e = G.gobblet_v1.env()
    e.reset()
    for a in (18, 36):
        e.last()
        e.step(a)
    obs, *_ = e.last()
    assert obs["action_mask"][18] == 0  # piece 3 is covered now
    before = e.unwrapped.board.squares.copy()
    e.step(18)
    assert np.array_equal(e.unwrapped.board.squares, before)
    assert e.terminations == {"player_1": True, "player_2": True} == e.truncations
    assert e.rewards == {"player_1": -1.0, "player_2": 0}
    with pytest.raises(AssertionError):
        G.gobblet_v1.env().reset() or e.step(54)


def test_text_render_matches_reference(capsys, golden_dir):
    """render_mode "text" / "text_full" (gobblet.py:299-429), character for character."""
    frames = json.load(open(os.path.join(golden_dir, "render_text.json")))
    g = np.load(os.path.join(golden_dir, "random_games.npz"))
    for mode in ("text", "text_full"):
        e = G.gobblet_v1.raw_env(render_mode=mode)
        for fr in [f for f in frames if f["mode"] == mode]:
            i = fr["index"]
            if g["ply"][i] == 0:
                e.reset()
            capsys.readouterr()
            e.step(int(g["action"][i]))
            assert capsys.readouterr().out == fr["text"], (mode, i)


def test_seed_determinism_like_pettingzoo_seed_test():
    """What pettingzoo.test.seed_test checks (reference tests/test_gobblet_env.py:45-50): two environments
    driven by the same seeded action stream produce identical observations, rewards and terminations."""
    def play(seed):
        rng = np.random.default_rng(seed)
        e = G.gobblet_v1.env()
        e.reset(seed=seed)
        trace = []
        for agent in e.agent_iter(max_iter=60):
            obs, reward, term, trunc, info = e.last()
            trace.append((agent, obs["observation"].tobytes(), obs["action_mask"].tobytes(), reward, term, trunc))
            if term or trunc:
                e.step(None)
            else:
                m = obs["action_mask"]
                e.step(int(rng.choice(np.flatnonzero(m))))
        return trace
    assert play(42) == play(42)
    assert play(42) != play(43)


def test_api_contract_like_pettingzoo_api_test():
    """The parts of pettingzoo.test.api_test (reference tests/test_gobblet_env.py:32-34) that concern this
    environment: observations / masks lie in their spaces with the declared dtype and shape, rewards and
    termination dicts cover exactly the live agents, actions are Discrete(54), dead agents step with None."""
    e = G.gobblet_v1.env()
    e.reset()
    assert e.possible_agents == ["player_1", "player_2"] and e.agents == e.possible_agents
    assert e.action_space("player_1").n == 54
    rng = np.random.default_rng(1)
    for agent in e.agent_iter():
        obs, reward, term, trunc, info = e.last()
        assert e.observation_space(agent).contains(obs)
        assert obs["observation"].dtype == np.int8 and obs["observation"].shape == (3, 3, 13)
        assert obs["action_mask"].dtype == np.int8 and obs["action_mask"].shape == (54,)
        assert set(e.rewards) == set(e.agents) == set(e.terminations) == set(e.truncations) == set(e.infos)
        if term or trunc:
            with pytest.raises(ValueError):
                e.unwrapped._was_dead_step(3)  # a dead agent may only pass None
            e.step(None)
        else:
            e.step(int(rng.choice(np.flatnonzero(obs["action_mask"]))))
    assert e.agents == []


def _norm_np_repr(text):
    """numpy >= 2 prints scalars inside lists as np.int64(4); numpy 1.x (the reference's pin) as 4"""
    return re.sub(r"np\.int64\((-?\d+)\)", r"\1", text)


def test_print_pieces_and_debug_render_match_reference(capsys, golden_dir):
    """Board.print_pieces / print / __str__ (board.py:155-156, 223-242) and render() with args.debug
    (gobblet.py:315-317) against stdout captured from the reference."""
    import types
    ref = json.load(open(os.path.join(golden_dir, "print_pieces.json")))
    for rec in ref["boards"]:
        b = G.gobblet_v1.Board(squares=rec["squares"])
        for key, fn in (("print_pieces", b.print_pieces), ("print", b.print), ("str", lambda: print(str(b)))):
            capsys.readouterr()
            fn()
            assert _norm_np_repr(capsys.readouterr().out) == _norm_np_repr(rec[key]), (rec["index"], key)
    g = np.load(os.path.join(golden_dir, "random_games.npz"))
    e = G.gobblet_v1.raw_env(render_mode="text", args=types.SimpleNamespace(debug=True))
    for fr in ref["debug_frames"]:
        i = fr["index"]
        if g["ply"][i] == 0:
            e.reset()
        capsys.readouterr()
        e.step(int(g["action"][i]))
        assert _norm_np_repr(capsys.readouterr().out) == _norm_np_repr(fr["text"]), i


def test_facade_has_no_public_backend_switch():
    import inspect
    for fn in (G.gobblet_v1.env, G.gobblet_v1.raw_env.__init__, G.gobblet_v1.Board.__init__):
        assert not [p for p in inspect.signature(fn).parameters if "backend" in p]
    assert G.gobblet_v1.raw_env.metadata["is_parallelizable"] is True  # gobblet.py:127


def test_parallel_env_cycles(oracle_engine):
    """parallel_env (gobblet.py:120) = PettingZoo's AEC -> parallel conversion of env(), restated (PARITY UNPINNED: the
    conversion is third-party and upstream skips its own test of it).  A cycle lets both agents move once: boards, masks and
    summed rewards must equal the AEC environment stepped twice; a win by the first mover leaves the second agent dead
    (its action must be None, as PettingZoo demands of a dead agent), and the episode ends with no agents."""
    par, aec = G.gobblet_v1.parallel_env(), G.gobblet_v1.env()
    obs = par.reset()
    aec.reset()
    assert set(obs) == {"player_1", "player_2"} and par.agents == ["player_1", "player_2"]
    rng = np.random.default_rng(3)
    for _ in range(3):  # three quiet cycles: small pieces on free squares, nobody can have a line yet
        acts = {}
        for a in par.agents:
            m = aec.observe(a)["action_mask"]
            acts[a] = int(rng.choice(np.flatnonzero(m[:18])))
            aec.step(acts[a])  # (the second mover chooses from its mask AFTER the first one's move)
        o, r, term, trunc, info = par.step(acts)
        if any(term.values()):
            break
        assert np.array_equal(par.unwrapped.board.squares, aec.unwrapped.board.squares)
        assert all(np.array_equal(o[a]["action_mask"], aec.observe(a)["action_mask"]) for a in par.agents)
        assert r == {"player_1": 0, "player_2": 0} and not any(trunc.values())
    # player_1 completes the line (0, 1, 2) with its third move (action = 9 * piece + square): the cycle ends the episode
    quiet = [{"player_1": 0, "player_2": 4}, {"player_1": 19, "player_2": 23}]
    par.reset()
    for acts in quiet:
        o, r, term, trunc, info = par.step(acts)
        assert not any(term.values())
    with pytest.raises(ValueError, match="dead"):  # the conversion hands player_2's action to a dead agent
        par.step({"player_1": 38, "player_2": 8})
    par.reset()
    for acts in quiet:
        par.step(acts)
    o, r, term, trunc, info = par.step({"player_1": 38, "player_2": None})
    assert r == {"player_1": 1, "player_2": -1} and all(term.values()) and par.agents == []


def _check_debug_illegal_frames(G, capsys, golden_dir, **envkw):
    """raw_env.step's debug branch (gobblet.py:238-242) frame by frame against stdout captured from the reference along
    games WITH illegal plies -- including the quirk that the branch's legality test is always player_2's (the agent name
    is passed as agent_index) -- and the board after every ply (illegal: unchanged, the turn passes)."""
    import types
    ref = json.load(open(os.path.join(golden_dir, "debug_illegal.json")))
    frames = ref["frames"]
    assert sum("--ERROR-- ILLEGAL MOVE" in f["text"] for f in frames) >= 20
    assert any(f["legal_for_mover"] and "--ERROR--" in f["text"] for f in frames)          # a legal move flagged
    assert any(not f["legal_for_mover"] and "--ERROR--" not in f["text"] for f in frames)  # an illegal move not flagged
    e = G.gobblet_v1.raw_env(render_mode="text", args=types.SimpleNamespace(debug=True), **envkw)
    for fr in frames:
        if fr["ply"] == 0:
            e.reset()
        assert e.agents.index(e.agent_selection) == fr["agent"]
        capsys.readouterr()
        e.step(fr["action"])
        assert _norm_np_repr(capsys.readouterr().out) == _norm_np_repr(fr["text"]), (fr["game"], fr["ply"])
        assert np.array_equal(np.asarray(e.board.squares).astype(int), np.asarray(fr["squares"])), (fr["game"], fr["ply"])
    for name, args in (("default", None), ("explicit", types.SimpleNamespace(screen_width=480))):  # gobblet.py:165-166
        env = G.gobblet_v1.raw_env(render_mode=None, args=args, **envkw)
        assert {"screen_width": env.screen_width, "screen_height": env.screen_height} == ref["attrs"][name]


def test_debug_branch_with_illegal_plies_matches_reference(capsys, golden_dir):
    _check_debug_illegal_frames(G, capsys, golden_dir)


def test_placement_search_logic(monkeypatch):
    """placement.spread_pair with a scripted probe, allocator and memory gauge (no GPU): either array is the head of a
    block of its own; it stops at the first clean pair, otherwise takes the best pair it saw, alternates which array gets
    a new block, honours the probe budget and the memory cap (64 GiB, a quarter of what was free at entry), ends quietly
    when the device refuses a block, refuses to start when not even the arrays' own blocks fit, probes a new block
    against one representative unless that pair is in between, and returns zero-filled arrays of the sizes asked for."""
    import weakref

    import torch
    from gobblet_rl_amd import placement
    GIB = placement.GIB

    made = []
    state = {"free": 288 * GIB, "refuse_after": None}

    def alloc(nbytes):
        if state["refuse_after"] is not None and len(made) >= state["refuse_after"]:
            raise MemoryError("scripted out-of-memory")
        made.append(nbytes)
        state["free"] -= nbytes
        t = torch.full((4096,), len(made), dtype=torch.uint8)  # (a stand-in for the block; the value tells which)
        weakref.finalize(t, give_back, nbytes)                 # (a block that is dropped goes back to the "driver")
        return t

    def give_back(nbytes):
        state["free"] += nbytes

    def run(ratios, free=288 * GIB, refuse_after=None, **kw):
        made.clear()
        state.update(free=free, refuse_after=refuse_after)
        script, seen = list(ratios), []

        def fake_probe(a, b, slot_boards=0, plies=0):
            seen.append((int(a[0]), int(b[0]), slot_boards, plies))
            r = script.pop(0) if script else 1.0
            return 100.0 * r, 60.0, 40.0

        monkeypatch.setattr(placement, "probe", fake_probe)
        kw.setdefault("far", False)  # (the far candidates have their own cases below)
        a, b, info = placement.spread_pair(1000, 500, "cpu", alloc=alloc, free=lambda: state["free"], **kw)
        assert a.numel() == 1000 and b.numel() == 500 and int(a.max()) == 0 and int(b.max()) == 0
        assert all(m >= placement.MIN_BLOCK_BYTES and m % placement.BLOCK_GRANULE == 0 for m in made)
        assert info["cap_gib"] <= placement.MAX_HOLD_BYTES / GIB and (kw["far"] or info["held_gib"] <= info["cap_gib"])
        return seen, info

    assert placement.block_bytes(1) == 2 << 30 and placement.block_bytes((2 << 30) + 1) == (2 << 30) + (2 << 20)
    assert placement.block_bytes(5 << 30) == 5 << 30
    seen, info = run([0.80])                              # clean at once: one probe, two blocks
    assert seen == [(1, 2, 0, 0)] and info["probes"] == [0.8] and info["held_gib"] == 4.0 and info["spread"]
    assert info["ended"] == "clean pair" and info["released_blocks"] == 0
    seen, info = run([1.0, 0.99, 1.0, 0.81], slot_boards=1024, plies=8)
    # after every plain conflict a gap (allocations 3, 5, 7: 2, 4, 8 GiB), then a new mask block (4), a new observation
    # block (6), a new mask block (8): each against the other array's first block
    assert [s[:2] for s in seen] == [(1, 2), (1, 4), (6, 2), (1, 8)] and all(s[2:] == (1024, 8) for s in seen)
    assert [m >> 30 for m in made] == [2, 2, 2, 2, 4, 2, 8, 2]
    assert info["ratio"] == 0.81 and info["spread"] and len(info["probes"]) == 4 and info["held_gib"] == 24.0
    assert info["released_blocks"] == 6
    seen, info = run([1.0, 0.94, 0.93])                   # in between: no gap, and the new block also meets the other blocks
    assert [s[:2] for s in seen][:4] == [(1, 2), (1, 4), (5, 2), (5, 4)]
    seen, info = run([1.0] * 60, max_probes=60)           # never clean: the memory cap (64 GiB) ends the search, best = first
    assert info["ratio"] == 1.0 and not info["spread"] and info["cap_gib"] == 64.0 and info["ended"].startswith("memory budget")
    assert sum(made) <= placement.MAX_HOLD_BYTES and max(made) <= placement.MAX_SKIP_BYTES
    seen, info = run([0.95] * 40)                         # never clean, never a plain conflict: the probe budget ends it
    assert len(seen) == placement.MAX_PROBES and info["ratio"] == 0.95 and info["ended"] == "probe budget"
    seen, info = run([1.0, 0.97, 0.9, 0.95, 0.99], max_probes=5)
    assert info["ratio"] == 0.9 and info["spread"] and len(seen) == 5
    seen, info = run([1.0] * 40, max_hold_bytes=10 << 30)  # an explicit cap: one gap fits, then blocks only
    assert len(seen) == 3 and info["held_gib"] == 10.0
    # a device that is mostly taken: the cap is a quarter of what is free
    seen, info = run([1.0] * 40, free=40 * GIB)
    assert info["cap_gib"] == 10.0 and info["held_gib"] <= 10.0 and sum(made) <= 10 * GIB
    # ... and the reserve stays untouched however small the blocks
    seen, info = run([1.0] * 40, free=9 * GIB)
    assert sum(made) <= 9 * GIB - placement.RESERVE_BYTES and info["cap_gib"] == 4.0   # (the arrays' own blocks always count)
    # the device refuses a block in mid-search: the search ends with what it has
    seen, info = run([1.0] * 40, refuse_after=4)
    assert info["ended"] == "the device refused a block" and len(made) == 4 and info["ratio"] == 1.0
    # not even the arrays' own blocks: the caller is told to allocate as it otherwise would
    with pytest.raises(placement.PlacementUnavailable):
        run([0.8], free=7 * GIB)
    with pytest.raises(placement.PlacementUnavailable):
        run([0.8], refuse_after=1)
    assert made == [2 << 30]
    # a device that is all ours hands out ONE class for 62 GiB on end (the driver's box, round 4): the capped search finds nothing,
    # then a candidate behind a transient gap of 64 GiB is still in the class, the one behind 96 GiB is clean
    near = len(run([1.0] * 40)[0])                        # (probes of the capped search when nothing is clean)
    seen, info = run([1.0] * near + [1.0, 0.81], far=True)
    assert info["ratio"] == 0.81 and info["spread"] and info["far_gaps_gib"] == [64, 96] and "transient gap of 96 GiB" in info["ended"]
    assert [m >> 30 for m in made][-4:] == [64, 2, 96, 2] and seen[-1][0] == 1   # (gap, block) twice; against the first observation block
    seen, info = run([1.0] * 40, far=True)                # nothing anywhere: three far candidates, then the best seen
    assert info["far_gaps_gib"] == [64, 96, 128] and info["ratio"] == 1.0 and not info["spread"]
    assert info["transient_peak_gib"] >= 128 + 2          # (what was held for the duration of two allocations is on record)
    seen, info = run([1.0] * 40, free=150 * GIB, far=None)  # a device that is not mostly free, nobody asked: no far candidates
    assert info["far_gaps_gib"] == [] and max(made) <= placement.MAX_SKIP_BYTES and info["transient_peak_gib"] == 0.0
    seen, info = run([1.0] * 40, free=288 * GIB, far=None)  # ... mostly free: tried unasked (the driver's box of round 4)
    assert info["far_gaps_gib"] == [64, 96, 128]
    seen, info = run([1.0] * 40, free=150 * GIB, far=True)  # the caller owns the device and says so: whatever gap still fits
    assert info["far_gaps_gib"] == [64, 96, 128]
    seen, info = run([1.0] * 40, free=100 * GIB, far=True)
    assert info["far_gaps_gib"] == [64] and 64 + 2 <= info["transient_peak_gib"] <= 100 - placement.RESERVE_BYTES / GIB
    # the pair as the caller's allocator places it is probed first and stays in the race
    plain_made = []

    def plain():
        plain_made.append(1)
        return torch.full((1000,), 77, dtype=torch.uint8), torch.full((500,), 78, dtype=torch.uint8)

    seen, info = run([0.80], plain=plain)                 # clean as it is: no block at all
    assert seen == [(77, 78, 0, 0)] and made == [] and info["ended"] == "the allocator's own placement is clean" and info["spread"]
    seen, info = run([1.0, 1.0, 0.81], plain=plain)       # not clean: the block search runs and wins
    assert [s[:2] for s in seen] == [(77, 78), (1, 2), (1, 4)] and info["ratio"] == 0.81 and info["probes"] == [1.0, 1.0, 0.81]
    seen, info = run([0.90] + [0.89] * 40, plain=plain)   # nothing clearly better turns up: the caller's own pair is kept
    assert info["ratio"] == 0.9 and "was not beaten" in info["ended"] and info["block_gib"] == [0.0, 0.0]
    seen, info = run([1.0], plain=plain, free=7 * GIB)    # no memory for blocks: no search, the plain pair, the reason recorded
    assert made == [] and info["ended"].startswith("no block search") and info["ratio"] == 1.0
